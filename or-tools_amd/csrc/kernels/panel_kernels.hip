// Column dots of [A | I] against a panel of K vectors in one pass over A
// (tableau rows and row combinations, include/mi_lp.h mi_lp_row_combinations).
//
// Every result is CompactSparseMatrix::ColumnScalarProduct (lp_data/sparse.h:
// 514-542) of one column and one vector: four strided accumulators r1..r4
// from +0.0, ((r1 + r2) + r3) + r4, then the <= 3 tail terms in order, every
// product and sum rounded separately (-ffp-contract=off). These kernels
// restate column_dot_kernel / dense_dot_kernel (simplex_kernels.hip) for K
// vectors; the order of the terms of one (column, vector) pair is theirs.
//
// The vectors are row-interleaved, Y[r * K + v], so the K values a matrix
// entry meets are contiguous. Results go to out[col * K + v] (a column's K
// results contiguous); deinterleave_kernel turns that into the caller's
// vector-major rows. Only vectors v < kp are stored (the others are padding).
//
// The sparse form (panel_count / panel_offsets / panel_write, at the end)
// filters out[col * K + v] by a column mask and a drop tolerance and packs
// the kept (column, value) pairs per vector in increasing column order; it
// replaces deinterleave_kernel when the caller wants sparse rows. The
// branching penalties (penalties_tile / penalties_fold, after it) reduce
// out[col * K + v] to one 32-byte record per vector instead, and the Gomory
// cuts (gomory_transform_tile / gomory_combine_tile / gomory_fold, after
// them) turn it into cut coefficients around a second pass of the dot
// kernels, which the sparse form then packs.
//
// The other direction, row sums [A | I] x for a panel of K points
// (row_sums_panel_kernel and the kernels that build its interleaved points:
// interleave, panel_fill, panel_override), follows the sparse form, and its
// own sparse form (violations_count / violations_fold / violations_write:
// the rows outside their bounds and one summary per point) comes after it.
// Last, the activity ranges of the rows under a panel of K bound sets
// (activity_ranges_panel_kernel), whose screening form goes through the same
// count, fold and write passes under a second rule, and the implied column
// bounds over those ranges (implied_bounds_panel_short_kernel /
// implied_bounds_panel_long_kernel: the column direction again, over the row
// direction's result), whose filtered form goes through them under a third;
// and what turns a round of them into the next (propagate_apply_panel_kernel,
// propagate_changed_keys_kernel: bound propagation to a fixpoint).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "block_scan.h"
#include "kernel_args.h"

namespace milp_kernels {

namespace {
typedef double dbl2 __attribute__((ext_vector_type(2)));
constexpr int kDenseColsPerBlock = 64;
}  // namespace

// ---------------------------------------------------------------------------
// Short columns: lane = slot * 4K + v * 4 + c owns vector v and chain c of its
// column and walks the chain sequentially, as quad_column_dot does (K = 1 is
// that function). A wave holds 64 / 4K columns: one at K = 16, four at K = 4.
// A step of a column reads 4 matrix entries (each by K lanes: a broadcast)
// and 4 x K contiguous doubles of Y.
template <int K>
__global__ __launch_bounds__(256) void column_dot_panel_short_kernel(PanelDotArgs a) {
  constexpr int kLanesPerCol = 4 * K;
  const int lane = threadIdx.x & 63;
  const int sub = threadIdx.x % kLanesPerCol;
  const int v = sub >> 2;
  const int c = sub & 3;
  const int col_slot = blockIdx.x * (256 / kLanesPerCol) + threadIdx.x / kLanesPerCol;
  // The lanes of a column stay converged through the shuffles: out-of-range
  // slots walk an empty range and skip the store.
  const bool in_range = col_slot < a.ncols;
  const int slot = in_range ? col_slot : 0;
  const int col = a.col_list != nullptr ? a.col_list[slot] : slot;
  const int64_t s = a.starts[col];
  const int64_t e = in_range ? a.starts[col + 1] : s;
  const int64_t len = e - s;
  const int64_t full = (len >= 4) ? (len / 4) * 4 : 0;
  const double* __restrict__ y = a.y + v;
  double acc = 0.0;
  for (int64_t i = s + c; i < s + full; i += 4) {
    acc += a.vals[i] * y[static_cast<int64_t>(a.rows[i]) * K];
  }
  const int g = lane & ~3;
  const double r1 = __shfl(acc, g + 0, kWave);
  const double r2 = __shfl(acc, g + 1, kWave);
  const double r3 = __shfl(acc, g + 2, kWave);
  const double r4 = __shfl(acc, g + 3, kWave);
  double result = r1 + r2 + r3 + r4;
  for (int64_t i = s + full; i < e; ++i) {
    result += a.vals[i] * y[static_cast<int64_t>(a.rows[i]) * K];
  }
  if (c == 0 && in_range && v < a.kp) a.out[static_cast<int64_t>(col) * K + v] = result;
}

// ---------------------------------------------------------------------------
// Long columns: one wave (one workgroup) per column, wave_column_dot's
// structure with K products per lane. The 64 lanes load 64 consecutive
// entries (coalesced) and the K contiguous Y values of their rows; the 64 x K
// products go through LDS (prod[v][entry], rows padded against bank
// conflicts), and lane v * 4 + c folds chain c of vector v in entry order.
constexpr int kPanelProdStride = 68;

template <int K>
__global__ __launch_bounds__(64) void column_dot_panel_long_kernel(PanelDotArgs a) {
  __shared__ double prod[K * kPanelProdStride];
  const int lane = threadIdx.x;
  const int v = (lane >> 2) % K;  // lanes >= 4K repeat a vector and never store
  const int c = lane & 3;
  const int slot = blockIdx.x;  // < ncols: the grid is exactly ncols workgroups
  const int col = a.col_list != nullptr ? a.col_list[slot] : slot;
  const int64_t s = a.starts[col];
  const int64_t e = a.starts[col + 1];
  const int64_t len = e - s;
  const int64_t full = (len >= 4) ? (len / 4) * 4 : 0;
  double acc = 0.0;
  for (int64_t base = 0; base < full; base += kWave) {
    const int64_t idx = base + lane;
    if (idx < full) {
      const double x = a.vals[s + idx];
      const double* __restrict__ yr = a.y + static_cast<int64_t>(a.rows[s + idx]) * K;
#pragma unroll
      for (int u = 0; u < K; ++u) prod[u * kPanelProdStride + lane] = x * yr[u];
    }
    __syncthreads();
    const int64_t nvalid = (full - base) < kWave ? (full - base) : kWave;
    const int nt = static_cast<int>(nvalid >> 2);  // terms of each chain in this chunk
    for (int t = 0; t < nt; ++t) acc += prod[v * kPanelProdStride + (t << 2) + c];
    __syncthreads();
  }
  const int g = lane & ~3;
  const double r1 = __shfl(acc, g + 0, kWave);
  const double r2 = __shfl(acc, g + 1, kWave);
  const double r3 = __shfl(acc, g + 2, kWave);
  const double r4 = __shfl(acc, g + 3, kWave);
  double result = r1 + r2 + r3 + r4;
  for (int64_t i = s + full; i < e; ++i) {
    result += a.vals[i] * a.y[static_cast<int64_t>(a.rows[i]) * K + v];
  }
  if (c == 0 && lane < 4 * K && v < a.kp) a.out[static_cast<int64_t>(col) * K + v] = result;
}

// ---------------------------------------------------------------------------
// Dense block (layout in kernel_args.h DenseArgs): dense_dot_kernel with K
// accumulators per lane. A workgroup owns 64 dense columns, wave k streams
// chain k of them with contiguous 1-KiB steps. The chain index is
// wave-uniform and the K y-values of a row are contiguous, so they come from
// scalar loads. The 4 x K partial sums of a column meet in LDS; wave k then
// folds vectors k, k + 4, ...: ((r1 + r2) + r3) + r4 and the <= 3 tail terms.
template <int K, int UNROLL>
__global__ __launch_bounds__(256) void dense_dot_panel_kernel(PanelDenseArgs a) {
  __shared__ double part[4][K][kDenseColsPerBlock];
  const int lane = threadIdx.x & 63;
  const int k = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // chain of this wave
  const int j = blockIdx.x * kDenseColsPerBlock + lane;
  const int nd = a.nd;
  const bool in_range = j < nd;
  const int steps = a.m >> 2;
  const int pairs = steps >> 1;
  double acc[K];
#pragma unroll
  for (int v = 0; v < K; ++v) acc[v] = 0.0;
  if (in_range) {
    const dbl2* __restrict__ p =
        reinterpret_cast<const dbl2*>(a.body) + static_cast<int64_t>(k) * nd + j;
    const double* __restrict__ y = a.y + static_cast<int64_t>(k) * K;
    const int64_t stride = static_cast<int64_t>(nd) * 4;  // double2 per pair step
    int t = 0;
    for (; t + UNROLL <= pairs; t += UNROLL) {
      dbl2 x[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) x[u] = __builtin_nontemporal_load(p + (t + u) * stride);
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const double* __restrict__ y0 = y + static_cast<int64_t>(t + u) * 8 * K;
        const double* __restrict__ y1 = y0 + 4 * K;
#pragma unroll
        for (int v = 0; v < K; ++v) {
          acc[v] += x[u].x * y0[v];
          acc[v] += x[u].y * y1[v];
        }
      }
    }
    for (; t < pairs; ++t) {
      const dbl2 x = p[t * stride];
      const double* __restrict__ y0 = y + static_cast<int64_t>(t) * 8 * K;
      const double* __restrict__ y1 = y0 + 4 * K;
#pragma unroll
      for (int v = 0; v < K; ++v) {
        acc[v] += x.x * y0[v];
        acc[v] += x.y * y1[v];
      }
    }
    if (steps & 1) {
      const double x = a.body[static_cast<int64_t>(pairs) * nd * 8 +
                              static_cast<int64_t>(k) * nd + j];
      const double* __restrict__ y0 = y + static_cast<int64_t>(steps - 1) * 4 * K;
#pragma unroll
      for (int v = 0; v < K; ++v) acc[v] += x * y0[v];
    }
  }
#pragma unroll
  for (int v = 0; v < K; ++v) part[k][v][lane] = acc[v];
  __syncthreads();
  if (!in_range) return;
  const int col = a.dense_cols[j];
  const int base = steps * 4;
  for (int v = k; v < K && v < a.kp; v += 4) {
    double result = part[0][v][lane] + part[1][v][lane] + part[2][v][lane] + part[3][v][lane];
    for (int r = 0; base + r < a.m; ++r) {
      result += a.tail[static_cast<int64_t>(r) * nd + j] *
                a.y[static_cast<int64_t>(base + r) * K + v];
    }
    a.out[static_cast<int64_t>(col) * K + v] = result;
  }
}

// out[v * ld + col] = in[col * K + v] for v < kp: a workgroup moves 64 columns
// through LDS, so that both sides are contiguous.
template <int K>
__global__ __launch_bounds__(256) void deinterleave_kernel(const double* __restrict__ in,
                                                           int ncols, int kp,
                                                           double* __restrict__ out,
                                                           int64_t ld) {
  __shared__ double tile[64 * (K + 1)];
  const int c0 = blockIdx.x * 64;
  const int cols = min(64, ncols - c0);
  for (int i = threadIdx.x; i < cols * K; i += 256) {
    tile[(i / K) * (K + 1) + i % K] = in[static_cast<int64_t>(c0) * K + i];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * kp; i += 256) {
    const int v = i >> 6;
    const int cl = i & 63;
    if (cl < cols) out[v * ld + c0 + cl] = tile[cl * (K + 1) + v];
  }
}

// ---------------------------------------------------------------------------
// Sparse rows out of the interleaved panel result, in three launches on one
// stream; no workgroup waits for another.
//   panel_count    a workgroup owns a tile of kPanelTileColumns consecutive
//                  columns and counts the kept entries of every vector in it:
//                  counts[v * tiles + tile].
//   panel_offsets  one workgroup turns the counts into where each (vector,
//                  tile) starts in the packed output, vector v right after
//                  v - 1, and writes the per-vector totals.
//   panel_write    the count kernel's tiles again: the kept entries of
//                  (vector, tile) go to cols / vals from that start on, in
//                  increasing column order.
// The tile's kPanelTileColumns * K doubles are contiguous in `in`; thread t
// reads elements t, t + 256, ... (coalesced). K divides 256, so a thread
// meets one vector only, v = t % K, at columns t / K + j * (256 / K).

// The keep rule of both kernels: the column passes the mask and |x| exceeds
// the tolerance. The comparison is false for a NaN and for +-0.0 at tolerance
// 0, true for +-inf unless the tolerance is +inf.
__device__ __forceinline__ bool panel_keep(double x, bool masked_in, double drop_tolerance) {
  return masked_in && fabs(x) > drop_tolerance;
}

__device__ __forceinline__ bool panel_mask_bit(const uint64_t* __restrict__ mask, int col) {
  return mask == nullptr || ((mask[col >> 6] >> (col & 63)) & 1ull) != 0;
}

template <int K>
__global__ __launch_bounds__(kPanelTileColumns) void panel_count_kernel(PanelSparseArgs a) {
  static_assert(kPanelTileColumns == 256 && kPanelTileColumns % K == 0 && kWave % K == 0,
                "a thread owns one vector");
  __shared__ int cnt[K];
  const int t = threadIdx.x;
  const int tile = blockIdx.x;
  const int col0 = tile * kPanelTileColumns;
  const int cols = min(kPanelTileColumns, a.ncols - col0);
  if (t < K) cnt[t] = 0;
  __syncthreads();
  const double* __restrict__ in = a.in + static_cast<int64_t>(col0) * K;
  const int v = t % K;
  int c = 0;
  if (v < a.kp) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int cl = t / K + j * (kPanelTileColumns / K);
      if (cl < cols) {
        const double x = in[t + j * kPanelTileColumns];
        c += panel_keep(x, panel_mask_bit(a.mask, col0 + cl), a.drop_tolerance) ? 1 : 0;
      }
    }
  }
  // Lanes l, l + K, l + 2K, ... of a wave hold the same vector.
#pragma unroll
  for (int off = K; off < kWave; off <<= 1) c += __shfl_xor(c, off, kWave);
  if ((t & (kWave - 1)) < K && v < a.kp) atomicAdd(&cnt[v], c);
  __syncthreads();
  if (t < a.kp) a.counts[static_cast<int64_t>(t) * a.tiles + tile] = cnt[t];
}

// offsets[v * tiles + tile] = kept entries of the vectors before v + those of
// v's tiles before `tile`; totals[v] = v's kept entries. One workgroup: per
// vector, a block scan per step of kPanelOffsetsStep tiles with the running
// total carried in a register (every thread computes the same one).
__global__ __launch_bounds__(kPanelOffsetsStep) void panel_offsets_kernel(PanelSparseArgs a) {
  __shared__ int lds_waves[kPanelOffsetsStep / kWave];
  const int t = threadIdx.x;
  int64_t running = 0;
  for (int v = 0; v < a.kp; ++v) {
    const int64_t begin = running;
    const int64_t row = static_cast<int64_t>(v) * a.tiles;
    for (int base = 0; base < a.tiles; base += kPanelOffsetsStep) {
      const int tile = base + t;
      const int c = tile < a.tiles ? a.counts[row + tile] : 0;
      int total;
      const int excl = scan_block_exclusive<kPanelOffsetsStep>(c, &total, lds_waves);
      if (tile < a.tiles) a.offsets[row + tile] = running + excl;
      running += total;
      __syncthreads();  // the next scan goes through the same lds_waves
    }
    if (t == 0) a.totals[v] = running - begin;
  }
}

// The tile is transposed through LDS, tile[v][column], so that a wave then
// reads 64 consecutive columns of one vector. Row stride: the ds_write_b64 of
// the staging pass is served in groups of 16 lanes over 32 banks, and a group
// holds 16 / K columns of K vectors each, at dword 2 * (v * stride + column):
// stride = 257 (K = 16) and 260 (K = 4) give every lane of a group its own
// bank pair; the row reads are consecutive doubles and conflict-free at any
// stride. Wave w then takes the vectors w, w + 4, ... < kp: per 64 columns a
// ballot of the keep rule, rank = the kept lanes below + the kept columns of
// the chunks before. The rule is the caller's, keep(x, column): the sparse
// rows and the violated rows (below) share the pass.
template <int K>
constexpr int panel_write_stride() {
  return kPanelTileColumns + (K == 1 ? 0 : 16 / K);
}

template <int K, typename Keep>
__device__ __forceinline__ void panel_write_tile(const double* __restrict__ in_all, int ncols,
                                                 int kp, int tiles,
                                                 const int64_t* __restrict__ offsets, Keep keep_rule,
                                                 int32_t* __restrict__ out_cols,
                                                 double* __restrict__ out_vals,
                                                 double* tile_vals) {
  constexpr int kStride = panel_write_stride<K>();
  const int t = threadIdx.x;
  const int tile = blockIdx.x;
  const int col0 = tile * kPanelTileColumns;
  const int cols = min(kPanelTileColumns, ncols - col0);
  const double* __restrict__ in = in_all + static_cast<int64_t>(col0) * K;
  {
    const int v = t % K;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int cl = t / K + j * (kPanelTileColumns / K);
      if (cl < cols && v < kp) tile_vals[v * kStride + cl] = in[t + j * kPanelTileColumns];
    }
  }
  __syncthreads();
  const int lane = t & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(t / kWave);
  for (int v = wave; v < kp; v += kPanelTileColumns / kWave) {
    int64_t pos = offsets[static_cast<int64_t>(v) * tiles + tile];
    for (int chunk = 0; chunk * kWave < cols; ++chunk) {
      const int cl = chunk * kWave + lane;
      double x = 0.0;
      bool keep = false;
      if (cl < cols) {
        x = tile_vals[v * kStride + cl];
        keep = keep_rule(x, col0 + cl);
      }
      const unsigned long long kept = __ballot(keep);
      if (keep) {
        const int64_t at = pos + __popcll(kept & ((1ull << lane) - 1ull));
        out_cols[at] = col0 + cl;
        out_vals[at] = x;
      }
      pos += __popcll(kept);
    }
  }
}

template <int K>
__global__ __launch_bounds__(kPanelTileColumns) void panel_write_kernel(PanelSparseArgs a) {
  __shared__ double tile_vals[K * panel_write_stride<K>()];
  panel_write_tile<K>(
      a.in, a.ncols, a.kp, a.tiles, a.offsets,
      [&a](double x, int col) {
        return panel_keep(x, panel_mask_bit(a.mask, col), a.drop_tolerance);
      },
      a.cols, a.vals, tile_vals);
}

// ---------------------------------------------------------------------------
// Branching penalties out of the interleaved panel result (include/mi_lp.h
// mi_lp_row_penalties has the rule), in two launches on one stream; they
// replace deinterleave_kernel when the caller wants one record per vector.
//   penalties_tile  panel_count_kernel's tile and thread layout: thread t
//                   reads elements t, t + 256, ... and meets one vector only,
//                   v = t % K, at columns t / K + j * (256 / K), ascending in
//                   j. Per direction it keeps (minimum, column, count) in
//                   registers; the lanes of a vector combine by shuffles, the
//                   four waves through LDS: one partial per (vector,
//                   direction, tile).
//   penalties_fold  workgroup v folds vector v's partials into its record.
// (minimum, column) partials merge to the smaller candidate and, among equal
// candidates, the lower column. A candidate is >= +0.0 and never NaN, so the
// merge is exact and symmetric: the result does not depend on the reduction
// tree. Without a column a partial is (+inf, kNoPenaltyColumn): a +inf
// candidate at a real column replaces it.
__device__ __forceinline__ void penalty_merge(double* value, int* col, double other_value,
                                              int other_col) {
  if (other_value < *value || (other_value == *value && other_col < *col)) {
    *value = other_value;
    *col = other_col;
  }
}

// One direction's candidate of an eligible column: dist * (cost / |alpha|),
// at least cost * unit for an integer column, every operation rounded on its
// own; a NaN (0 * inf, inf / inf) counts as +0.0.
__device__ __forceinline__ double penalty_candidate(double cost, double abs_alpha, double dist,
                                                    double unit) {
  const double r = cost / abs_alpha;
  double c = dist * r;
  if (unit > 0.0) {
    const double step = cost * unit;
    c = c < step ? step : c;
  }
  return c != c ? 0.0 : c;
}

template <int K>
__global__ __launch_bounds__(kPanelTileColumns) void penalties_tile_kernel(PenaltyArgs a) {
  static_assert(kPanelTileColumns == 256 && kPanelTileColumns % K == 0 && kWave % K == 0,
                "a thread owns one vector");
  constexpr int kWaves = kPanelTileColumns / kWave;
  __shared__ double wave_min[kWaves][2][K];
  __shared__ int wave_col[kWaves][2][K];
  __shared__ int wave_count[kWaves][2][K];
  const int t = threadIdx.x;
  const int tile = blockIdx.x;
  const int col0 = tile * kPanelTileColumns;
  const int cols = min(kPanelTileColumns, a.ncols - col0);
  const double* __restrict__ in = a.in + static_cast<int64_t>(col0) * K;
  const int v = t % K;
  double best[2] = {__builtin_inf(), __builtin_inf()};
  int best_col[2] = {kNoPenaltyColumn, kNoPenaltyColumn};
  int count[2] = {0, 0};
  if (v < a.kp) {
    const double dist[2] = {a.down_dist[v], a.up_dist[v]};
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int cl = t / K + j * (kPanelTileColumns / K);
      if (cl < cols) {
        const int col = col0 + cl;
        const double alpha = in[t + j * kPanelTileColumns];
        const int status = a.status[col];
        if (status == 0 || status == 1) continue;  // MI_LP_BASIC, MI_LP_FIXED_VALUE
        const double d = a.d[col];
        const double unit = a.unit != nullptr ? a.unit[col] : 0.0;
        const bool at_lower = status == 2;  // MI_LP_AT_LOWER_BOUND
        const bool at_upper = status == 3;  // MI_LP_AT_UPPER_BOUND
        const bool is_free = !at_lower && !at_upper;  // MI_LP_FREE
        const double cost = at_lower ? (d > 0.0 ? d : 0.0) : (at_upper ? (d < 0.0 ? -d : 0.0) : 0.0);
        bool eligible[2];
        double candidate[2];
        if (alpha != alpha || d != d) {
          eligible[0] = eligible[1] = true;
          candidate[0] = candidate[1] = 0.0;
        } else {
          const double abs_alpha = fabs(alpha);
          if (!(abs_alpha > a.pivot_tolerance)) continue;
          const bool positive = alpha > 0.0;
          eligible[0] = is_free || (at_lower && positive) || (at_upper && !positive);
          eligible[1] = is_free || (at_lower && !positive) || (at_upper && positive);
#pragma unroll
          for (int dir = 0; dir < 2; ++dir) {
            candidate[dir] = penalty_candidate(cost, abs_alpha, dist[dir], unit);
          }
        }
#pragma unroll
        for (int dir = 0; dir < 2; ++dir) {
          if (eligible[dir]) {
            ++count[dir];
            penalty_merge(&best[dir], &best_col[dir], candidate[dir], col);
          }
        }
      }
    }
  }
  // Lanes l, l + K, l + 2K, ... of a wave hold the same vector.
#pragma unroll
  for (int off = K; off < kWave; off <<= 1) {
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
      count[dir] += __shfl_xor(count[dir], off, kWave);
      const double other = __shfl_xor(best[dir], off, kWave);
      const int other_col = __shfl_xor(best_col[dir], off, kWave);
      penalty_merge(&best[dir], &best_col[dir], other, other_col);
    }
  }
  const int lane = t & (kWave - 1);
  const int wave = t / kWave;
  if (lane < K) {  // lane == v
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
      wave_min[wave][dir][lane] = best[dir];
      wave_col[wave][dir][lane] = best_col[dir];
      wave_count[wave][dir][lane] = count[dir];
    }
  }
  __syncthreads();
  if (t < 2 * K && t % K < a.kp) {  // thread (direction t / K, vector t % K)
    const int dir = t / K;
    double value = wave_min[0][dir][v];
    int col = wave_col[0][dir][v];
    int c = wave_count[0][dir][v];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      c += wave_count[w][dir][v];
      penalty_merge(&value, &col, wave_min[w][dir][v], wave_col[w][dir][v]);
    }
    const int64_t at = static_cast<int64_t>(v * 2 + dir) * a.tiles + tile;
    a.tile_min[at] = value;
    a.tile_col[at] = col;
    a.tile_count[at] = c;
  }
}

// Workgroup v folds vector v's tile partials of both directions into its
// record: the smallest candidate, the lowest column attaining it (-1 without
// one) and the integer sum of the counts (at most ncols < 2^31).
__global__ __launch_bounds__(kPanelOffsetsStep) void penalties_fold_kernel(PenaltyArgs a) {
  constexpr int kWaves = kPanelOffsetsStep / kWave;
  __shared__ double wave_min[kWaves][2];
  __shared__ int wave_col[kWaves][2];
  __shared__ int wave_count[kWaves][2];
  const int t = threadIdx.x;
  const int v = blockIdx.x;  // < kp: the grid is exactly kp workgroups
  double best[2] = {__builtin_inf(), __builtin_inf()};
  int best_col[2] = {kNoPenaltyColumn, kNoPenaltyColumn};
  int count[2] = {0, 0};
#pragma unroll
  for (int dir = 0; dir < 2; ++dir) {
    const int64_t base = static_cast<int64_t>(v * 2 + dir) * a.tiles;
    for (int tile = t; tile < a.tiles; tile += kPanelOffsetsStep) {
      count[dir] += a.tile_count[base + tile];
      penalty_merge(&best[dir], &best_col[dir], a.tile_min[base + tile], a.tile_col[base + tile]);
    }
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      count[dir] += __shfl_xor(count[dir], off, kWave);
      const double other = __shfl_xor(best[dir], off, kWave);
      const int other_col = __shfl_xor(best_col[dir], off, kWave);
      penalty_merge(&best[dir], &best_col[dir], other, other_col);
    }
    if ((t & (kWave - 1)) == 0) {
      wave_min[t / kWave][dir] = best[dir];
      wave_col[t / kWave][dir] = best_col[dir];
      wave_count[t / kWave][dir] = count[dir];
    }
  }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
#pragma unroll
      for (int w = 1; w < kWaves; ++w) {
        count[dir] += wave_count[w][dir];
        penalty_merge(&best[dir], &best_col[dir], wave_min[w][dir], wave_col[w][dir]);
      }
    }
    BranchPenalty r;
    r.down = best[0];
    r.up = best[1];
    r.down_col = best_col[0] == kNoPenaltyColumn ? -1 : best_col[0];
    r.up_col = best_col[1] == kNoPenaltyColumn ? -1 : best_col[1];
    r.down_count = count[0];
    r.up_count = count[1];
    a.out[v] = r;
  }
}

// ---------------------------------------------------------------------------
// Gomory mixed-integer cuts out of the interleaved panel result (include/
// mi_lp.h mi_lp_row_gomory_cuts has the rule), around a second pass of the
// dot kernels; penalties_tile's tile and thread layout throughout.
//   gomory_transform_tile  alpha -> g per (column, vector) over all N columns.
//                          The structural part goes to a buffer of its own;
//                          the slack part IS the vector y' of the second dot
//                          pass (the slack of row r is -(A x)_r), stored
//                          row-interleaved where the dot kernels read y: slack
//                          column n + r of the tile lands at element
//                          (col - n) * K + v, contiguous like the load.
//   (dot pass)             s = y'^T A, into the panel result again.
//   gomory_combine_tile    c = g - s over the n structural columns, in place,
//                          and the per-tile partials of the summary over the
//                          entries with fabs(c) > drop_tolerance.
//   gomory_fold            workgroup v folds vector v's partials.
// The extrema merge to the larger (smaller) value and, among equal values,
// the lower column; the counts are integer sums: exact and symmetric, the
// same bits in any reduction order.
__device__ __forceinline__ void cut_merge_max(double* value, int* col, double other_value,
                                              int other_col) {
  if (other_value > *value || (other_value == *value && other_col < *col)) {
    *value = other_value;
    *col = other_col;
  }
}

// Steps 1-6 of the rule for one (column, vector); every operation rounded on
// its own. *bad counts a NaN alpha and a FREE column above the tolerance.
__device__ __forceinline__ double gomory_coefficient(double alpha, int status, double unit,
                                                     double f0, double row_unit,
                                                     double zero_tolerance, int* bad) {
  if (status == 0 || status == 1) return 0.0;  // MI_LP_BASIC, MI_LP_FIXED_VALUE
  if (alpha != alpha) {
    ++*bad;
    return 0.0;
  }
  if (!(fabs(alpha) > zero_tolerance)) return 0.0;
  if (status == 4) {  // MI_LP_FREE
    ++*bad;
    return 0.0;
  }
  const bool at_lower = status == 2;  // MI_LP_AT_LOWER_BOUND; else MI_LP_AT_UPPER_BOUND
  const double abar = at_lower ? alpha : -alpha;
  double gamma;
  if (unit > 0.0) {
    const double scaled = abar * unit;
    const double t = scaled / row_unit;
    const double f = t - floor(t);
    gamma = f <= f0 ? f / f0 : (1.0 - f) / (1.0 - f0);
    gamma = gamma / unit;
  } else {
    const double t = abar / row_unit;
    gamma = t > 0.0 ? t / f0 : (-t) / (1.0 - f0);
  }
  return at_lower ? gamma : 0.0 - gamma;
}

template <int K>
__global__ __launch_bounds__(kPanelTileColumns) void gomory_transform_tile_kernel(GomoryArgs a) {
  static_assert(kPanelTileColumns == 256 && kPanelTileColumns % K == 0 && kWave % K == 0,
                "a thread owns one vector");
  constexpr int kWaves = kPanelTileColumns / kWave;
  __shared__ int wave_bad[kWaves][K];
  const int t = threadIdx.x;
  const int tile = blockIdx.x;
  const int col0 = tile * kPanelTileColumns;
  const int cols = min(kPanelTileColumns, a.ncols - col0);
  const double* __restrict__ in = a.cols + static_cast<int64_t>(col0) * K;
  const int v = t % K;
  const bool live = v < a.kp;
  const double f0 = live ? a.f0[v] : 0.5;
  const double row_unit = live ? a.row_unit[v] : 1.0;
  int bad = 0;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const int cl = t / K + j * (kPanelTileColumns / K);
    if (cl < cols) {
      const int col = col0 + cl;
      double g = 0.0;  // the padding slots v >= kp
      if (live) {
        const double alpha = in[t + j * kPanelTileColumns];
        const int status = a.status[col];
        const double unit = a.unit != nullptr ? a.unit[col] : 0.0;
        g = gomory_coefficient(alpha, status, unit, f0, row_unit, a.zero_tolerance, &bad);
      }
      if (col < a.n) {
        a.g[static_cast<int64_t>(col) * K + v] = g;
      } else {
        a.slack[static_cast<int64_t>(col - a.n) * K + v] = g;
      }
    }
  }
  // Lanes l, l + K, l + 2K, ... of a wave hold the same vector.
#pragma unroll
  for (int off = K; off < kWave; off <<= 1) bad += __shfl_xor(bad, off, kWave);
  const int lane = t & (kWave - 1);
  if (lane < K) wave_bad[t / kWave][lane] = bad;  // lane == v
  __syncthreads();
  if (t < K && t < a.kp) {
    int sum = wave_bad[0][t];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) sum += wave_bad[w][t];
    a.tile_bad[static_cast<int64_t>(t) * a.tiles + tile] = sum;
  }
}

template <int K>
__global__ __launch_bounds__(kPanelTileColumns) void gomory_combine_tile_kernel(GomoryArgs a) {
  static_assert(kPanelTileColumns == 256 && kPanelTileColumns % K == 0 && kWave % K == 0,
                "a thread owns one vector");
  constexpr int kWaves = kPanelTileColumns / kWave;
  __shared__ double wave_max[kWaves][K];
  __shared__ double wave_min[kWaves][K];
  __shared__ int wave_max_col[kWaves][K];
  __shared__ int wave_min_col[kWaves][K];
  __shared__ int wave_count[kWaves][K];
  __shared__ int wave_nan[kWaves][K];
  const int t = threadIdx.x;
  const int tile = blockIdx.x;
  const int col0 = tile * kPanelTileColumns;
  const int cols = min(kPanelTileColumns, a.n - col0);
  double* __restrict__ s = a.cols + static_cast<int64_t>(col0) * K;
  const double* __restrict__ g = a.g + static_cast<int64_t>(col0) * K;
  const int v = t % K;
  double hi = 0.0;
  double lo = __builtin_inf();
  int hi_col = kNoCutColumn;
  int lo_col = kNoCutColumn;
  int count = 0;
  int nan = 0;
  if (v < a.kp) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int cl = t / K + j * (kPanelTileColumns / K);
      if (cl < cols) {
        const int at = t + j * kPanelTileColumns;
        const double c = g[at] - s[at];
        s[at] = c;
        const double abs_c = fabs(c);
        if (c != c) ++nan;
        if (abs_c > a.drop_tolerance) {  // panel_keep's rule without a mask
          ++count;
          cut_merge_max(&hi, &hi_col, abs_c, col0 + cl);
          penalty_merge(&lo, &lo_col, abs_c, col0 + cl);
        }
      }
    }
  }
#pragma unroll
  for (int off = K; off < kWave; off <<= 1) {
    count += __shfl_xor(count, off, kWave);
    nan += __shfl_xor(nan, off, kWave);
    const double other_hi = __shfl_xor(hi, off, kWave);
    const int other_hi_col = __shfl_xor(hi_col, off, kWave);
    cut_merge_max(&hi, &hi_col, other_hi, other_hi_col);
    const double other_lo = __shfl_xor(lo, off, kWave);
    const int other_lo_col = __shfl_xor(lo_col, off, kWave);
    penalty_merge(&lo, &lo_col, other_lo, other_lo_col);
  }
  const int lane = t & (kWave - 1);
  const int wave = t / kWave;
  if (lane < K) {  // lane == v
    wave_max[wave][lane] = hi;
    wave_min[wave][lane] = lo;
    wave_max_col[wave][lane] = hi_col;
    wave_min_col[wave][lane] = lo_col;
    wave_count[wave][lane] = count;
    wave_nan[wave][lane] = nan;
  }
  __syncthreads();
  if (t < K && t < a.kp) {
    hi = wave_max[0][t];
    lo = wave_min[0][t];
    hi_col = wave_max_col[0][t];
    lo_col = wave_min_col[0][t];
    count = wave_count[0][t];
    nan = wave_nan[0][t];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      count += wave_count[w][t];
      nan += wave_nan[w][t];
      cut_merge_max(&hi, &hi_col, wave_max[w][t], wave_max_col[w][t]);
      penalty_merge(&lo, &lo_col, wave_min[w][t], wave_min_col[w][t]);
    }
    const int64_t at = static_cast<int64_t>(t) * a.tiles_n + tile;
    a.tile_count[at] = count;
    a.tile_nan[at] = nan;
    a.tile_max[at] = hi;
    a.tile_min[at] = lo;
    a.tile_max_col[at] = hi_col;
    a.tile_min_col[at] = lo_col;
  }
}

// Workgroup v folds vector v's partials of both kernels into its summary:
// integer sums (at most ncols < 2^31 each), the exact extrema and the lowest
// column attaining each (-1 without a kept entry).
__global__ __launch_bounds__(kPanelOffsetsStep) void gomory_fold_kernel(GomoryArgs a) {
  constexpr int kWaves = kPanelOffsetsStep / kWave;
  __shared__ double wave_max[kWaves];
  __shared__ double wave_min[kWaves];
  __shared__ int wave_max_col[kWaves];
  __shared__ int wave_min_col[kWaves];
  __shared__ int wave_count[kWaves];
  __shared__ int wave_bad[kWaves];
  const int t = threadIdx.x;
  const int v = blockIdx.x;  // < kp: the grid is exactly kp workgroups
  double hi = 0.0;
  double lo = __builtin_inf();
  int hi_col = kNoCutColumn;
  int lo_col = kNoCutColumn;
  int count = 0;
  int bad = 0;
  const int64_t base_all = static_cast<int64_t>(v) * a.tiles;
  for (int tile = t; tile < a.tiles; tile += kPanelOffsetsStep) bad += a.tile_bad[base_all + tile];
  const int64_t base = static_cast<int64_t>(v) * a.tiles_n;
  for (int tile = t; tile < a.tiles_n; tile += kPanelOffsetsStep) {
    count += a.tile_count[base + tile];
    bad += a.tile_nan[base + tile];
    cut_merge_max(&hi, &hi_col, a.tile_max[base + tile], a.tile_max_col[base + tile]);
    penalty_merge(&lo, &lo_col, a.tile_min[base + tile], a.tile_min_col[base + tile]);
  }
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    count += __shfl_xor(count, off, kWave);
    bad += __shfl_xor(bad, off, kWave);
    const double other_hi = __shfl_xor(hi, off, kWave);
    const int other_hi_col = __shfl_xor(hi_col, off, kWave);
    cut_merge_max(&hi, &hi_col, other_hi, other_hi_col);
    const double other_lo = __shfl_xor(lo, off, kWave);
    const int other_lo_col = __shfl_xor(lo_col, off, kWave);
    penalty_merge(&lo, &lo_col, other_lo, other_lo_col);
  }
  if ((t & (kWave - 1)) == 0) {
    wave_max[t / kWave] = hi;
    wave_min[t / kWave] = lo;
    wave_max_col[t / kWave] = hi_col;
    wave_min_col[t / kWave] = lo_col;
    wave_count[t / kWave] = count;
    wave_bad[t / kWave] = bad;
  }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      count += wave_count[w];
      bad += wave_bad[w];
      cut_merge_max(&hi, &hi_col, wave_max[w], wave_max_col[w]);
      penalty_merge(&lo, &lo_col, wave_min[w], wave_min_col[w]);
    }
    CutSummary r;
    r.max_abs = hi;
    r.min_abs = lo;
    r.count = count;
    r.bad_count = bad;
    r.max_col = hi_col == kNoCutColumn ? -1 : hi_col;
    r.min_col = lo_col == kNoCutColumn ? -1 : lo_col;
    a.out[v] = r;
  }
}

// ---------------------------------------------------------------------------
// Row sums [A | I] x for a panel of K points in one pass over the rows
// (include/mi_lp.h mi_lp_column_combinations): row_sum_kernel's sum
// (simplex_kernels.hip; variable_values.cc:101-131, sparse.h:389-399) for K
// points, without mask and sign. Per (row, point): from +0.0, the row's
// entries in increasing column order, acc = acc + x[col] * a, an entry whose
// multiplier is +-0.0 left out, every product and sum rounded separately.
//
// The points are column-interleaved, X[col * K + v]. Thread t owns the pair
// (row t / K of the workgroup's 256 / K rows, point t % K) and walks the row
// strictly in order. The K lanes of a row are adjacent: an entry's (col, val)
// is one address for all of them and its K multipliers are one contiguous
// read (128 B at K = 16). The entries are read directly: a row's lanes stream
// it front to back, so each of its cache lines is fetched once. The gathers
// of kRowPanelUnroll entries are issued before the ordered adds that consume
// them. A skipped term is added as -0.0, which leaves every sum's bits
// unchanged (x + -0.0 == x, also for x = +-0.0) and the lanes converged.
template <int K>
__global__ __launch_bounds__(kRowPanelThreads) void row_sums_panel_kernel(RowPanelArgs a) {
  static_assert(kRowPanelThreads % K == 0, "whole rows per workgroup");
  constexpr int kRows = kRowPanelThreads / K;
  const int v = threadIdx.x % K;
  const int row = blockIdx.x * kRows + threadIdx.x / K;
  if (row >= a.num_rows) return;  // no barrier and no cross-lane step below
  const int64_t s = a.t_starts[row];
  const int64_t e = a.t_starts[row + 1];
  const double* __restrict__ x = a.x + v;
  double acc = 0.0;
  int64_t i = s;
  for (; i + kRowPanelUnroll <= e; i += kRowPanelUnroll) {
    int col[kRowPanelUnroll];
    double val[kRowPanelUnroll];
    double mult[kRowPanelUnroll];
#pragma unroll
    for (int u = 0; u < kRowPanelUnroll; ++u) {
      col[u] = a.t_cols[i + u];
      val[u] = a.t_vals[i + u];
    }
#pragma unroll
    for (int u = 0; u < kRowPanelUnroll; ++u) mult[u] = x[static_cast<int64_t>(col[u]) * K];
#pragma unroll
    for (int u = 0; u < kRowPanelUnroll; ++u) acc += mult[u] != 0.0 ? mult[u] * val[u] : -0.0;
  }
  for (; i < e; ++i) {
    const double mult = x[static_cast<int64_t>(a.t_cols[i]) * K];
    acc += mult != 0.0 ? mult * a.t_vals[i] : -0.0;
  }
  if (v < a.kp) a.out[static_cast<int64_t>(row) * K + v] = acc;
}

// out[col * K + v] = in[v * ld + col] for v < kp and 0.0 for the padding
// points: deinterleave_kernel backwards, 64 columns through LDS so that both
// sides are contiguous.
template <int K>
__global__ __launch_bounds__(256) void interleave_kernel(const double* __restrict__ in,
                                                         int64_t ld, int ncols, int kp,
                                                         double* __restrict__ out) {
  __shared__ double tile[64 * (K + 1)];
  const int c0 = blockIdx.x * 64;
  const int cols = min(64, ncols - c0);
  for (int i = threadIdx.x; i < 64 * kp; i += 256) {
    const int v = i >> 6;
    const int cl = i & 63;
    if (cl < cols) tile[cl * (K + 1) + v] = in[v * ld + c0 + cl];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cols * K; i += 256) {
    const int v = i % K;
    out[static_cast<int64_t>(c0) * K + i] = v < kp ? tile[(i / K) * (K + 1) + v] : 0.0;
  }
}

// out[col * K + v] = base[col] for v < kp and 0.0 for the padding points.
template <int K>
__global__ __launch_bounds__(256) void panel_fill_kernel(const double* __restrict__ base,
                                                         int ncols, int kp,
                                                         double* __restrict__ out) {
  const int64_t total = static_cast<int64_t>(ncols) * K;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < total; i += stride) {
    out[i] = static_cast<int>(i % K) < kp ? base[i / K] : 0.0;
  }
}

// Override i of the panel belongs to the point v with starts[v] <= i <
// starts[v + 1] (at most 16 points: a linear search).
template <int K>
__global__ __launch_bounds__(256) void panel_override_kernel(RowPanelOverrideArgs a) {
  const int64_t first = a.starts[0];
  const int64_t last = a.starts[a.kp];
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
  for (int64_t i = first + static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < last;
       i += stride) {
    int v = 0;
    while (v + 1 < a.kp && a.starts[v + 1] <= i) ++v;
    a.x[static_cast<int64_t>(a.cols[i]) * K + v] = a.vals[i];
  }
}

// ---------------------------------------------------------------------------
// Violated rows and per-point summaries out of row_sums_panel_kernel's
// interleaved result (include/mi_lp.h mi_lp_column_combinations_violations),
// in the sparse rows' scheme: a count pass over tiles of kPanelTileColumns
// rows, panel_offsets_kernel as it is, a fold of the tile partials into the
// summaries, and the ordered write pass. Kernel boundaries on one stream are
// the only ordering; no workgroup waits for another.

// The keep rule of the count and the write pass. Both widened bounds are one
// rounded operation each (-ffp-contract=off); a NaN activity fails both
// comparisons and is violated.
__device__ __forceinline__ bool row_violated(double a, double lo, double hi, double tolerance) {
  return !(a >= lo - tolerance) || !(a <= hi + tolerance);
}

// The amount of a violated row: > 0 and never NaN (lo != +inf, hi != -inf
// and a violated +-inf activity has a finite or opposite bound on its side).
__device__ __forceinline__ double violation_amount(double a, double lo, double hi) {
  if (a != a) return __builtin_inf();
  const double below = lo - a;
  const double above = a - hi;
  return below > above ? below : above;
}

// (amount, row) partials: the larger amount, the lower row among equal
// amounts. Without a violated row a partial is (0.0, kNoWorstRow); every
// amount is > 0, so any violated row replaces it. Exact and symmetric: the
// result does not depend on the reduction tree.
constexpr int kNoWorstRow = 0x7fffffff;
__device__ __forceinline__ void worst_merge(double* amount, int* row, double other_amount,
                                            int other_row) {
  if (other_amount > *amount || (other_amount == *amount && other_row < *row)) {
    *amount = other_amount;
    *row = other_row;
  }
}

// The rule of the count and the write pass and the amount of a kept row, by
// PanelRowRule: the violated rows of row sums, or the rows whose g (formed by
// activity_ranges_panel_kernel) exceeds the tolerance. g is never NaN and a
// kept g is > tolerance >= 0, so worst_merge's (0.0, kNoWorstRow) start
// serves both.
template <int RULE>
struct RowRule;
template <>
struct RowRule<kRowRuleOutsideBounds> {
  static __device__ __forceinline__ bool keep(const RowViolationArgs& a, double x, int row,
                                              double* amount) {
    const double lo = a.row_lb[row];
    const double hi = a.row_ub[row];
    if (!row_violated(x, lo, hi, a.tolerance)) return false;
    *amount = violation_amount(x, lo, hi);
    return true;
  }
  static __device__ __forceinline__ bool keep(const RowViolationArgs& a, double x, int row) {
    return row_violated(x, a.row_lb[row], a.row_ub[row], a.tolerance);
  }
};
template <>
struct RowRule<kRowRuleAboveTolerance> {
  static __device__ __forceinline__ bool keep(const RowViolationArgs& a, double x, int,
                                              double* amount) {
    *amount = x;
    return x > a.tolerance;
  }
  static __device__ __forceinline__ bool keep(const RowViolationArgs& a, double x, int) {
    return x > a.tolerance;
  }
};
// The keys of implied_bounds_panel_kernel: kept when >= 0 (never NaN), and
// the key is the amount. An amount of 0.0 is a kept column that does not
// cross: worst_index() keeps it out of the merge's indices, since 0.0 at a
// real index would replace the (0.0, kNoWorstRow) start.
template <>
struct RowRule<kRowRuleKeptKey> {
  static __device__ __forceinline__ bool keep(const RowViolationArgs&, double x, int,
                                              double* amount) {
    *amount = x;
    return x >= 0.0;
  }
  static __device__ __forceinline__ bool keep(const RowViolationArgs&, double x, int) {
    return x >= 0.0;
  }
};
// The index a kept element enters the worst-merge with.
template <int RULE>
__device__ __forceinline__ int worst_index(double amount, int index) {
  if constexpr (RULE == kRowRuleKeptKey) return amount > 0.0 ? index : kNoWorstRow;
  return index;
}

// panel_count_kernel's tile and thread layout: thread t reads elements t,
// t + 256, ... of the tile's 256 * K contiguous doubles and meets one point
// only, v = t % K, at rows t / K + j * (256 / K), ascending in j. The lanes
// of a point combine by shuffles, the four waves through LDS.
template <int K, int RULE>
__global__ __launch_bounds__(kPanelTileColumns) void violations_count_kernel(
    RowViolationArgs a) {
  static_assert(kPanelTileColumns == 256 && kPanelTileColumns % K == 0 && kWave % K == 0,
                "a thread owns one point");
  constexpr int kWaves = kPanelTileColumns / kWave;
  __shared__ int wave_count[kWaves][K];
  __shared__ double wave_amount[kWaves][K];
  __shared__ int wave_row[kWaves][K];
  const int t = threadIdx.x;
  const int tile = blockIdx.x;
  const int row0 = tile * kPanelTileColumns;
  const int rows = min(kPanelTileColumns, a.num_rows - row0);
  const double* __restrict__ in = a.in + static_cast<int64_t>(row0) * K;
  const int v = t % K;
  int c = 0;
  double amount = 0.0;
  int worst_row = kNoWorstRow;
  if (v < a.kp) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int rl = t / K + j * (kPanelTileColumns / K);
      if (rl < rows) {
        const double x = in[t + j * kPanelTileColumns];
        double row_amount;
        if (RowRule<RULE>::keep(a, x, row0 + rl, &row_amount)) {
          ++c;
          worst_merge(&amount, &worst_row, row_amount, worst_index<RULE>(row_amount, row0 + rl));
        }
      }
    }
  }
  // Lanes l, l + K, l + 2K, ... of a wave hold the same point.
#pragma unroll
  for (int off = K; off < kWave; off <<= 1) {
    c += __shfl_xor(c, off, kWave);
    const double other_amount = __shfl_xor(amount, off, kWave);
    const int other_row = __shfl_xor(worst_row, off, kWave);
    worst_merge(&amount, &worst_row, other_amount, other_row);
  }
  const int lane = t & (kWave - 1);
  const int wave = t / kWave;
  if (lane < K) {  // lane == v
    wave_count[wave][lane] = c;
    wave_amount[wave][lane] = amount;
    wave_row[wave][lane] = worst_row;
  }
  __syncthreads();
  if (t < a.kp) {
    c = wave_count[0][t];
    amount = wave_amount[0][t];
    worst_row = wave_row[0][t];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      c += wave_count[w][t];
      worst_merge(&amount, &worst_row, wave_amount[w][t], wave_row[w][t]);
    }
    const int64_t at = static_cast<int64_t>(t) * a.tiles + tile;
    a.counts[at] = c;
    a.tile_worst[at] = amount;
    a.tile_worst_row[at] = worst_row;
  }
}

// Workgroup v folds point v's tile partials into its summary: the integer
// sum of the counts, the largest amount and the lowest row attaining it.
// kIndexOptional (kRowRuleKeptKey): kept elements may all be without an index,
// and the summary's worst_row is then -1 beside a count > 0.
template <bool kIndexOptional>
__global__ __launch_bounds__(kPanelOffsetsStep) void violations_fold_kernel(RowViolationArgs a) {
  constexpr int kWaves = kPanelOffsetsStep / kWave;
  __shared__ long long wave_count[kWaves];
  __shared__ double wave_amount[kWaves];
  __shared__ int wave_row[kWaves];
  const int t = threadIdx.x;
  const int v = blockIdx.x;  // < kp: the grid is exactly kp workgroups
  const int64_t base = static_cast<int64_t>(v) * a.tiles;
  long long c = 0;
  double amount = 0.0;
  int worst_row = kNoWorstRow;
  for (int tile = t; tile < a.tiles; tile += kPanelOffsetsStep) {
    c += a.counts[base + tile];
    worst_merge(&amount, &worst_row, a.tile_worst[base + tile], a.tile_worst_row[base + tile]);
  }
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    c += __shfl_xor(c, off, kWave);
    const double other_amount = __shfl_xor(amount, off, kWave);
    const int other_row = __shfl_xor(worst_row, off, kWave);
    worst_merge(&amount, &worst_row, other_amount, other_row);
  }
  if ((t & (kWave - 1)) == 0) {
    wave_count[t / kWave] = c;
    wave_amount[t / kWave] = amount;
    wave_row[t / kWave] = worst_row;
  }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      c += wave_count[w];
      worst_merge(&amount, &worst_row, wave_amount[w], wave_row[w]);
    }
    PointViolations s;
    s.count = c;
    const bool any = kIndexOptional ? worst_row != kNoWorstRow : c > 0;
    s.worst = any ? amount : 0.0;
    s.worst_row = any ? worst_row : -1;
    s.reserved = 0;
    a.summaries[v] = s;
  }
}

// panel_write_kernel's pass with the rule: rows[offset + rank] and
// activities[offset + rank] (the kept element of `in`: the activity, or g,
// which is its own amount) in increasing row order.
template <int K, int RULE>
__global__ __launch_bounds__(kPanelTileColumns) void violations_write_kernel(
    RowViolationArgs a) {
  __shared__ double tile_vals[K * panel_write_stride<K>()];
  panel_write_tile<K>(
      a.in, a.num_rows, a.kp, a.tiles, a.offsets,
      [&a](double x, int row) { return RowRule<RULE>::keep(a, x, row); }, a.rows, a.activities,
      tile_vals);
}

// ---------------------------------------------------------------------------
// Activity ranges of the rows of A under a panel of K bound sets in one pass
// over the rows (include/mi_lp.h mi_lp_bound_activity_ranges; the argument
// block says what is stored). row_sums_panel_kernel's shape: thread t owns
// (row t / K, child t % K), the K lanes of a row are adjacent, the row is
// walked strictly in order and the gathers of kRowPanelUnroll entries are
// issued ahead of the ordered adds; no barrier and no cross-lane step. An
// entry meets two contiguous reads of K doubles, L[col * K ..] and
// U[col * K ..]; which of them feeds the minimum depends on the sign of the
// entry, which is one value for the K lanes of a row but not for a wave, so
// it is a select and not a branch. The slack entry (col >= num_structural),
// a zero coefficient and an infinite bound are added as -0.0, which leaves
// every sum's bits unchanged, and the counts are incremented by the
// predicate: the lanes stay converged. The slack's gather is redirected to
// column 0 (the bound arrays end at num_structural columns).
__device__ __forceinline__ void activity_range_term(double a, double l, double u, bool structural,
                                                    double* lo, double* hi, int* lo_inf,
                                                    int* hi_inf) {
  const bool up = a > 0.0;  // false for a NaN coefficient: the else branch of the rule
  const double bl = up ? l : u;
  const double bh = up ? u : l;
  const bool live = structural && a != 0.0;
  const bool lo_is_inf = fabs(bl) == __builtin_inf();
  const bool hi_is_inf = fabs(bh) == __builtin_inf();
  *lo += (live && !lo_is_inf) ? a * bl : -0.0;
  *hi += (live && !hi_is_inf) ? a * bh : -0.0;
  *lo_inf += (live && lo_is_inf) ? 1 : 0;
  *hi_inf += (live && hi_is_inf) ? 1 : 0;
}

template <int K>
__global__ __launch_bounds__(kRowPanelThreads) void activity_ranges_panel_kernel(
    ActivityRangeArgs a) {
  static_assert(kRowPanelThreads % K == 0, "whole rows per workgroup");
  constexpr int kRows = kRowPanelThreads / K;
  const int v = threadIdx.x % K;
  const int row = blockIdx.x * kRows + threadIdx.x / K;
  if (row >= a.num_rows) return;  // no barrier and no cross-lane step below
  const int64_t s = a.t_starts[row];
  const int64_t e = a.t_starts[row + 1];
  const int n = a.num_structural;
  const double* __restrict__ lower = a.lower + v;
  const double* __restrict__ upper = a.upper + v;
  double lo = 0.0;
  double hi = 0.0;
  int lo_inf = 0;
  int hi_inf = 0;
  int64_t i = s;
  for (; i + kRowPanelUnroll <= e; i += kRowPanelUnroll) {
    int col[kRowPanelUnroll];
    double val[kRowPanelUnroll];
    double l[kRowPanelUnroll];
    double u[kRowPanelUnroll];
#pragma unroll
    for (int j = 0; j < kRowPanelUnroll; ++j) {
      col[j] = a.t_cols[i + j];
      val[j] = a.t_vals[i + j];
    }
#pragma unroll
    for (int j = 0; j < kRowPanelUnroll; ++j) {
      const int64_t at = static_cast<int64_t>(col[j] < n ? col[j] : 0) * K;
      l[j] = lower[at];
      u[j] = upper[at];
    }
#pragma unroll
    for (int j = 0; j < kRowPanelUnroll; ++j) {
      activity_range_term(val[j], l[j], u[j], col[j] < n, &lo, &hi, &lo_inf, &hi_inf);
    }
  }
  for (; i < e; ++i) {
    const int col = a.t_cols[i];
    const int64_t at = static_cast<int64_t>(col < n ? col : 0) * K;
    activity_range_term(a.t_vals[i], lower[at], upper[at], col < n, &lo, &hi, &lo_inf, &hi_inf);
  }
  if (v >= a.kp) return;
  const int64_t at = static_cast<int64_t>(row) * K + v;
  if (a.row_lb != nullptr) {
    // Each difference is one rounded operation; a NaN difference fails the
    // comparison and never replaces g.
    double g = -__builtin_inf();
    const double over = lo - a.row_ub[row];
    const double under = a.row_lb[row] - hi;
    if (lo_inf == 0 && over > g) g = over;
    if (hi_inf == 0 && under > g) g = under;
    a.out[at] = g;
  } else {
    const int64_t block = static_cast<int64_t>(a.num_rows) * K;
    a.out[at] = lo;
    a.out[block + at] = hi;
    reinterpret_cast<unsigned long long*>(a.out)[2 * block + at] =
        static_cast<unsigned long long>(static_cast<unsigned int>(lo_inf)) |
        (static_cast<unsigned long long>(static_cast<unsigned int>(hi_inf)) << 32);
  }
}

// ---------------------------------------------------------------------------
// Implied column bounds under a panel of K bound sets: one round of bound
// propagation over activity_ranges_panel_kernel's dense result
// (include/mi_lp.h mi_lp_bound_implied_bounds has the rule; the argument
// block says what is read and stored). The column direction: per entry (r, a)
// of a structural column, child v gathers lo[r * K + v], hi[r * K + v] and the
// packed counts at r * K + v (three contiguous reads of K words over the K
// lanes of a column) and the two row bounds, forms at most one candidate for
// each of its two bounds and keeps the largest lower and the smallest upper
// candidate. Every candidate is rounded on its own (a product, a difference,
// a difference, a quotient, + 0.0) and the result is a max and a min of them,
// so it has the same bits in any order: the two shapes below differ only in
// who walks which entries.
//
// One side of an entry: the row bound rb, the range sum s with cnt infinite
// terms, and the bound b that this column fed into s. No candidate unless rb
// is finite and either no term is infinite (the column's own term leaves the
// sum) or the column's own is the only one. + 0.0 turns a -0.0 quotient into
// +0.0, so that equal candidates have equal bits.
__device__ __forceinline__ void implied_candidate(double rb, double s, int cnt, double b, double a,
                                                  double* q, bool* ok) {
  const bool b_is_inf = fabs(b) == __builtin_inf();
  const double res = cnt == 0 ? s - a * b : s;
  const double quotient = (rb - res) / a;
  *ok = fabs(rb) < __builtin_inf() && (cnt == 0 || (cnt == 1 && b_is_inf)) &&
        fabs(quotient) < __builtin_inf();  // false for a NaN quotient
  *q = quotient + 0.0;
}

// The sign of `a` is one value for the K lanes of a column but not for a
// wave: selects, as in activity_range_term. The lo side (against row_ub)
// tightens the upper bound of a column with a > 0 and the lower bound
// otherwise; the hi side the other one. A zero or NaN entry gives nothing. A
// NaN own bound fails every comparison and stays.
__device__ __forceinline__ void implied_term(double a, double l, double u, double lo, double hi,
                                             unsigned long long counts, double rlb, double rub,
                                             double* nl, double* nu) {
  const bool live = a != 0.0 && a == a;
  const bool up = a > 0.0;
  const double bl = up ? l : u;
  const double bh = up ? u : l;
  double q_lo, q_hi;
  bool ok_lo, ok_hi;
  implied_candidate(rub, lo, static_cast<int>(counts & 0xffffffffull), bl, a, &q_lo, &ok_lo);
  implied_candidate(rlb, hi, static_cast<int>(counts >> 32), bh, a, &q_hi, &ok_hi);
  const double for_upper = up ? q_lo : q_hi;
  const double for_lower = up ? q_hi : q_lo;
  const bool upper_ok = live && (up ? ok_lo : ok_hi);
  const bool lower_ok = live && (up ? ok_hi : ok_lo);
  *nu = (upper_ok && for_upper < *nu) ? for_upper : *nu;
  *nl = (lower_ok && for_lower > *nl) ? for_lower : *nl;
}

// The results of (col, v) and, in list mode, its key (ImpliedBoundsArgs).
// Every difference is one rounded operation; inf - inf is NaN and fails its
// comparison.
__device__ __forceinline__ void implied_store(const ImpliedBoundsArgs& a, int col, int64_t at,
                                              double l, double u, double nl, double nu) {
  a.new_lower[at] = nl;
  a.new_upper[at] = nu;
  if (a.keys == nullptr) return;
  const bool moved = (nl - l > a.tolerance) || (u - nu > a.tolerance);
  const double cross = nl - nu;
  const bool crossing = cross > a.tolerance;
  bool changed = false;
  if (a.base_lb != nullptr) {
    changed = __double_as_longlong(l) != __double_as_longlong(a.base_lb[col]) ||
              __double_as_longlong(u) != __double_as_longlong(a.base_ub[col]);
  }
  a.keys[at] = crossing ? cross : ((moved || changed) ? 0.0 : -1.0);
}

// Short columns: thread t owns (column t / K of the workgroup's 256 / K,
// child t % K), as the row kernels own (row, child). The column is walked
// with the gathers of kRowPanelUnroll entries issued ahead of the compares;
// no LDS, no barrier and no cross-lane step. The padding children read the
// unwritten part of `ranges` and store nothing.
template <int K>
__global__ __launch_bounds__(kRowPanelThreads) void implied_bounds_panel_short_kernel(
    ImpliedBoundsArgs a) {
  static_assert(kRowPanelThreads % K == 0, "whole columns per workgroup");
  constexpr int kCols = kRowPanelThreads / K;
  const int v = threadIdx.x % K;
  const int col = blockIdx.x * kCols + threadIdx.x / K;
  if (col >= a.num_cols) return;
  const int64_t s = a.starts[col];
  const int64_t e = a.starts[col + 1];
  const int64_t block = static_cast<int64_t>(a.num_rows) * K;
  const double* __restrict__ lo_all = a.ranges + v;
  const double* __restrict__ hi_all = a.ranges + block + v;
  const unsigned long long* __restrict__ counts_all =
      reinterpret_cast<const unsigned long long*>(a.ranges) + 2 * block + v;
  const int64_t at = static_cast<int64_t>(col) * K + v;
  const double l = a.lower[at];
  const double u = a.upper[at];
  double nl = l;
  double nu = u;
  int64_t i = s;
  for (; i + kRowPanelUnroll <= e; i += kRowPanelUnroll) {
    int row[kRowPanelUnroll];
    double val[kRowPanelUnroll];
    double lo[kRowPanelUnroll];
    double hi[kRowPanelUnroll];
    unsigned long long counts[kRowPanelUnroll];
    double rlb[kRowPanelUnroll];
    double rub[kRowPanelUnroll];
#pragma unroll
    for (int j = 0; j < kRowPanelUnroll; ++j) {
      row[j] = a.rows[i + j];
      val[j] = a.vals[i + j];
    }
#pragma unroll
    for (int j = 0; j < kRowPanelUnroll; ++j) {
      const int64_t r = static_cast<int64_t>(row[j]) * K;
      lo[j] = lo_all[r];
      hi[j] = hi_all[r];
      counts[j] = counts_all[r];
      rlb[j] = a.row_lb[row[j]];
      rub[j] = a.row_ub[row[j]];
    }
#pragma unroll
    for (int j = 0; j < kRowPanelUnroll; ++j) {
      implied_term(val[j], l, u, lo[j], hi[j], counts[j], rlb[j], rub[j], &nl, &nu);
    }
  }
  for (; i < e; ++i) {
    const int row = a.rows[i];
    const int64_t r = static_cast<int64_t>(row) * K;
    implied_term(a.vals[i], l, u, lo_all[r], hi_all[r], counts_all[r], a.row_lb[row],
                 a.row_ub[row], &nl, &nu);
  }
  if (v >= a.kp) return;
  implied_store(a, col, at, l, u, nl, nu);
}

// Long columns: one workgroup per column. Thread t is child t % K and slice
// t / K of the 256 / K slices and walks the entries slice, slice + 256 / K,
// ...; every slice starts from the own bounds. The partials of a child fold
// by shuffles over the lanes l, l + K, l + 2K, ... of a wave and then over the
// four waves through LDS: a max and a min, exact in any order.
template <int K>
__global__ __launch_bounds__(kRowPanelThreads) void implied_bounds_panel_long_kernel(
    ImpliedBoundsArgs a) {
  static_assert(kRowPanelThreads % K == 0 && kWave % K == 0, "a thread owns one child");
  constexpr int kSlices = kRowPanelThreads / K;
  constexpr int kWaves = kRowPanelThreads / kWave;
  __shared__ double wave_lower[kWaves][K];
  __shared__ double wave_upper[kWaves][K];
  const int t = threadIdx.x;
  const int v = t % K;
  const int slice = t / K;
  const int col = blockIdx.x;  // < num_cols: the grid is exactly num_cols workgroups
  const int64_t s = a.starts[col];
  const int64_t e = a.starts[col + 1];
  const int64_t block = static_cast<int64_t>(a.num_rows) * K;
  const double* __restrict__ lo_all = a.ranges + v;
  const double* __restrict__ hi_all = a.ranges + block + v;
  const unsigned long long* __restrict__ counts_all =
      reinterpret_cast<const unsigned long long*>(a.ranges) + 2 * block + v;
  const int64_t at = static_cast<int64_t>(col) * K + v;
  const double l = a.lower[at];
  const double u = a.upper[at];
  double nl = l;
  double nu = u;
  for (int64_t i = s + slice; i < e; i += kSlices) {
    const int row = a.rows[i];
    const int64_t r = static_cast<int64_t>(row) * K;
    implied_term(a.vals[i], l, u, lo_all[r], hi_all[r], counts_all[r], a.row_lb[row],
                 a.row_ub[row], &nl, &nu);
  }
#pragma unroll
  for (int off = K; off < kWave; off <<= 1) {
    const double other_lower = __shfl_xor(nl, off, kWave);
    const double other_upper = __shfl_xor(nu, off, kWave);
    nl = other_lower > nl ? other_lower : nl;
    nu = other_upper < nu ? other_upper : nu;
  }
  const int lane = t & (kWave - 1);
  const int wave = t / kWave;
  if (lane < K) {  // lane == v
    wave_lower[wave][lane] = nl;
    wave_upper[wave][lane] = nu;
  }
  __syncthreads();
  if (t >= a.kp) return;  // t == v below
  nl = wave_lower[0][t];
  nu = wave_upper[0][t];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) {
    nl = wave_lower[w][t] > nl ? wave_lower[w][t] : nl;
    nu = wave_upper[w][t] < nu ? wave_upper[w][t] : nu;
  }
  implied_store(a, col, at, l, u, nl, nu);
}

// The two bounds at the kept columns of the kRowRuleKeptKey write pass
// (ImpliedGatherArgs): workgroup (x, v) takes entries x * 256 ... of child v.
template <int K>
__global__ __launch_bounds__(256) void implied_gather_kernel(ImpliedGatherArgs a) {
  const int v = blockIdx.y;  // < kp
  int64_t start = 0;
  for (int j = 0; j < v; ++j) start += a.totals[j];
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= a.totals[v]) return;
  const int64_t from = static_cast<int64_t>(a.cols[start + i]) * K + v;
  a.out_lower[start + i] = a.new_lower[from];
  a.out_upper[start + i] = a.new_upper[from];
}

// ---------------------------------------------------------------------------
// Bound propagation to a fixpoint (include/mi_lp.h mi_lp_bound_propagate has
// the rule): what turns one round's implied bounds into the next round's own
// bounds, on the interleaved layout. Thread i owns element i = col * K + v of
// four arrays (nl, nu, l, u) and of the keys: every access is coalesced, a
// thread reads and writes its own element only, and the launch comes after
// the phase-2 kernel that read l and u, so the update is in place. No LDS, no
// barrier, no atomics. Every difference and sum is one rounded operation
// (-ffp-contract=off); ceil and floor are exact; + 0.0 turns -0.0 into +0.0;
// an infinity and a NaN pass through all three unchanged.
template <int K>
__global__ __launch_bounds__(256) void propagate_apply_panel_kernel(PropagateApplyArgs a) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= static_cast<int64_t>(a.num_cols) * K) return;
  const int v = static_cast<int>(i % K);
  if (v >= a.kp) return;
  if ((a.frozen >> v) & 1u) {
    a.keys[i] = -1.0;
    if (a.moved_keys != nullptr) a.moved_keys[i] = -1.0;
    return;
  }
  double nl = a.new_lower[i];
  double nu = a.new_upper[i];
  const double l = a.lower[i];
  const double u = a.upper[i];
  if (a.is_integer != nullptr && a.is_integer[i / K] != 0) {
    nl = ceil(nl - a.integrality_tolerance) + 0.0;
    nu = floor(nu + a.integrality_tolerance) + 0.0;
  }
  // inf - inf is NaN and a NaN own bound gives NaN: neither is a move.
  const bool moved = (nl - l > a.tolerance) || (u - nu > a.tolerance);
  const double out_l = moved ? nl : l;
  const double out_u = moved ? nu : u;
  const double cross = out_l - out_u;
  const bool crossing = cross > a.tolerance;
  if (moved) {
    a.lower[i] = out_l;
    a.upper[i] = out_u;
  }
  a.keys[i] = crossing ? cross : (moved ? 0.0 : -1.0);
  if (a.moved_keys != nullptr) a.moved_keys[i] = moved ? 0.0 : -1.0;
}

// The keys of the propagated lists, same ownership: a set's final bounds
// against the base, in bits, and the crossing columns.
template <int K>
__global__ __launch_bounds__(256) void propagate_changed_keys_kernel(PropagateChangedArgs a) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= static_cast<int64_t>(a.num_cols) * K) return;
  if (static_cast<int>(i % K) >= a.kp) return;
  const double l = a.lower[i];
  const double u = a.upper[i];
  const int64_t col = i / K;
  const bool changed = __double_as_longlong(l) != __double_as_longlong(a.base_lb[col]) ||
                       __double_as_longlong(u) != __double_as_longlong(a.base_ub[col]);
  const double cross = l - u;
  a.keys[i] = cross > a.tolerance ? cross : (changed ? 0.0 : -1.0);
}

}  // namespace milp_kernels

namespace milp_launch {
using namespace milp_kernels;

static inline int panel_div_up(long a, long b) { return static_cast<int>((a + b - 1) / b); }

// launch(std::integral_constant<int, K>) for the panel width K = width, then
// the launch error. A width other than 1, 4 or 16 launches nothing.
template <typename Launch>
static hipError_t for_panel_width(int width, Launch launch) {
  switch (width) {
    case 1: launch(std::integral_constant<int, 1>()); break;
    case 4: launch(std::integral_constant<int, 4>()); break;
    case 16: launch(std::integral_constant<int, 16>()); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t column_dot_panel(int width, bool long_columns, const PanelDotArgs& args,
                            hipStream_t s) {
  if (args.ncols <= 0) return hipSuccess;
  return for_panel_width(width, [&](auto w) {
    constexpr int K = decltype(w)::value;
    if (long_columns) {
      column_dot_panel_long_kernel<K><<<args.ncols, 64, 0, s>>>(args);
    } else {
      const int blocks = panel_div_up(args.ncols, 256 / (4 * K));
      column_dot_panel_short_kernel<K><<<blocks, 256, 0, s>>>(args);
    }
  });
}

hipError_t dense_dot_panel(int width, const PanelDenseArgs& args, hipStream_t s) {
  if (args.nd <= 0) return hipSuccess;
  const int blocks = panel_div_up(args.nd, kDenseColsPerBlock);
  return for_panel_width(width, [&](auto w) {
    constexpr int K = decltype(w)::value;
    constexpr int kUnroll = K == 16 ? 4 : 8;
    dense_dot_panel_kernel<K, kUnroll><<<blocks, 256, 0, s>>>(args);
  });
}

hipError_t panel_deinterleave(int width, const double* in, int ncols, int kp, double* out,
                              int64_t ld, hipStream_t s) {
  if (ncols <= 0 || kp <= 0) return hipSuccess;
  const int blocks = panel_div_up(ncols, 64);
  return for_panel_width(width, [&](auto w) {
    deinterleave_kernel<decltype(w)::value><<<blocks, 256, 0, s>>>(in, ncols, kp, out, ld);
  });
}

hipError_t panel_sparse(int width, const PanelSparseArgs& args, hipStream_t s) {
  if (args.ncols <= 0 || args.kp <= 0) return hipSuccess;
  if (args.tiles != panel_div_up(args.ncols, kPanelTileColumns)) return hipErrorInvalidValue;
  return for_panel_width(width, [&](auto w) {
    constexpr int K = decltype(w)::value;
    panel_count_kernel<K><<<args.tiles, kPanelTileColumns, 0, s>>>(args);
    panel_offsets_kernel<<<1, kPanelOffsetsStep, 0, s>>>(args);
    panel_write_kernel<K><<<args.tiles, kPanelTileColumns, 0, s>>>(args);
  });
}

hipError_t panel_penalties(int width, const PenaltyArgs& args, hipStream_t s) {
  if (args.ncols <= 0 || args.kp <= 0) return hipSuccess;
  if (args.tiles != panel_div_up(args.ncols, kPanelTileColumns)) return hipErrorInvalidValue;
  return for_panel_width(width, [&](auto w) {
    constexpr int K = decltype(w)::value;
    penalties_tile_kernel<K><<<args.tiles, kPanelTileColumns, 0, s>>>(args);
    penalties_fold_kernel<<<args.kp, kPanelOffsetsStep, 0, s>>>(args);
  });
}

static bool gomory_args_ok(const GomoryArgs& args) {
  return args.n >= 0 && args.n <= args.ncols &&
         args.tiles == panel_div_up(args.ncols, kPanelTileColumns) &&
         args.tiles_n == panel_div_up(args.n, kPanelTileColumns);
}

hipError_t panel_gomory_transform(int width, const GomoryArgs& args, hipStream_t s) {
  if (args.ncols <= 0 || args.kp <= 0) return hipSuccess;
  if (!gomory_args_ok(args)) return hipErrorInvalidValue;
  return for_panel_width(width, [&](auto w) {
    gomory_transform_tile_kernel<decltype(w)::value>
        <<<args.tiles, kPanelTileColumns, 0, s>>>(args);
  });
}

hipError_t panel_gomory_combine(int width, const GomoryArgs& args, hipStream_t s) {
  if (args.ncols <= 0 || args.kp <= 0) return hipSuccess;
  if (!gomory_args_ok(args)) return hipErrorInvalidValue;
  return for_panel_width(width, [&](auto w) {
    if (args.tiles_n > 0) {
      gomory_combine_tile_kernel<decltype(w)::value>
          <<<args.tiles_n, kPanelTileColumns, 0, s>>>(args);
    }
    gomory_fold_kernel<<<args.kp, kPanelOffsetsStep, 0, s>>>(args);
  });
}

hipError_t row_sums_panel(int width, const RowPanelArgs& args, hipStream_t s) {
  if (args.num_rows <= 0 || args.kp <= 0) return hipSuccess;
  return for_panel_width(width, [&](auto w) {
    constexpr int K = decltype(w)::value;
    const int blocks = panel_div_up(args.num_rows, kRowPanelThreads / K);
    row_sums_panel_kernel<K><<<blocks, kRowPanelThreads, 0, s>>>(args);
  });
}

hipError_t activity_ranges_panel(int width, const ActivityRangeArgs& args, hipStream_t s) {
  if (args.num_rows <= 0 || args.kp <= 0) return hipSuccess;
  if ((args.row_lb == nullptr) != (args.row_ub == nullptr)) return hipErrorInvalidValue;
  return for_panel_width(width, [&](auto w) {
    constexpr int K = decltype(w)::value;
    const int blocks = panel_div_up(args.num_rows, kRowPanelThreads / K);
    activity_ranges_panel_kernel<K><<<blocks, kRowPanelThreads, 0, s>>>(args);
  });
}

hipError_t implied_bounds_panel(int width, bool long_columns, const ImpliedBoundsArgs& args,
                                hipStream_t s) {
  if (args.num_cols <= 0 || args.kp <= 0) return hipSuccess;
  if ((args.base_lb == nullptr) != (args.base_ub == nullptr)) return hipErrorInvalidValue;
  return for_panel_width(width, [&](auto w) {
    constexpr int K = decltype(w)::value;
    if (long_columns) {
      implied_bounds_panel_long_kernel<K><<<args.num_cols, kRowPanelThreads, 0, s>>>(args);
    } else {
      const int blocks = panel_div_up(args.num_cols, kRowPanelThreads / K);
      implied_bounds_panel_short_kernel<K><<<blocks, kRowPanelThreads, 0, s>>>(args);
    }
  });
}

hipError_t implied_gather(int width, const ImpliedGatherArgs& args, hipStream_t s) {
  if (args.num_cols <= 0 || args.kp <= 0) return hipSuccess;
  const dim3 grid(panel_div_up(args.num_cols, 256), args.kp);
  return for_panel_width(width, [&](auto w) {
    implied_gather_kernel<decltype(w)::value><<<grid, 256, 0, s>>>(args);
  });
}

hipError_t propagate_apply(int width, const PropagateApplyArgs& args, hipStream_t s) {
  if (args.num_cols <= 0 || args.kp <= 0) return hipSuccess;
  if (args.kp > 32) return hipErrorInvalidValue;  // `frozen` has 32 bits
  return for_panel_width(width, [&](auto w) {
    constexpr int K = decltype(w)::value;
    const int blocks = panel_div_up(static_cast<long>(args.num_cols) * K, 256);
    propagate_apply_panel_kernel<K><<<blocks, 256, 0, s>>>(args);
  });
}

hipError_t propagate_changed_keys(int width, const PropagateChangedArgs& args, hipStream_t s) {
  if (args.num_cols <= 0 || args.kp <= 0) return hipSuccess;
  return for_panel_width(width, [&](auto w) {
    constexpr int K = decltype(w)::value;
    const int blocks = panel_div_up(static_cast<long>(args.num_cols) * K, 256);
    propagate_changed_keys_kernel<K><<<blocks, 256, 0, s>>>(args);
  });
}

// launch(std::integral_constant<int, RULE>) for a PanelRowRule.
template <typename Launch>
static void for_row_rule(int rule, Launch launch) {
  if (rule == kRowRuleOutsideBounds) {
    launch(std::integral_constant<int, kRowRuleOutsideBounds>());
  } else if (rule == kRowRuleAboveTolerance) {
    launch(std::integral_constant<int, kRowRuleAboveTolerance>());
  } else {
    launch(std::integral_constant<int, kRowRuleKeptKey>());
  }
}

hipError_t row_violations_panel(int width, int rule, const RowViolationArgs& args,
                                hipStream_t s) {
  if (args.num_rows <= 0 || args.kp <= 0) return hipSuccess;
  if (args.tiles != panel_div_up(args.num_rows, kPanelTileColumns)) return hipErrorInvalidValue;
  if (rule != kRowRuleOutsideBounds && rule != kRowRuleAboveTolerance &&
      rule != kRowRuleKeptKey) {
    return hipErrorInvalidValue;
  }
  return for_panel_width(width, [&](auto w) {
    constexpr int K = decltype(w)::value;
    for_row_rule(rule, [&](auto r) {
      violations_count_kernel<K, decltype(r)::value>
          <<<args.tiles, kPanelTileColumns, 0, s>>>(args);
    });
    if (args.rows != nullptr) {
      PanelSparseArgs o{};  // the fields panel_offsets_kernel reads
      o.kp = args.kp;
      o.tiles = args.tiles;
      o.counts = args.counts;
      o.offsets = args.offsets;
      o.totals = args.totals;
      panel_offsets_kernel<<<1, kPanelOffsetsStep, 0, s>>>(o);
    }
    if (args.summaries != nullptr) {
      if (rule == kRowRuleKeptKey) {
        violations_fold_kernel<true><<<args.kp, kPanelOffsetsStep, 0, s>>>(args);
      } else {
        violations_fold_kernel<false><<<args.kp, kPanelOffsetsStep, 0, s>>>(args);
      }
    }
    if (args.rows != nullptr) {
      for_row_rule(rule, [&](auto r) {
        violations_write_kernel<K, decltype(r)::value>
            <<<args.tiles, kPanelTileColumns, 0, s>>>(args);
      });
    }
  });
}

hipError_t panel_interleave(int width, const double* in, int64_t ld, int ncols, int kp,
                            double* out, hipStream_t s) {
  if (ncols <= 0) return hipSuccess;
  const int blocks = panel_div_up(ncols, 64);
  return for_panel_width(width, [&](auto w) {
    interleave_kernel<decltype(w)::value><<<blocks, 256, 0, s>>>(in, ld, ncols, kp, out);
  });
}

// Grid-stride kernels: at most 2048 workgroups.
static inline int panel_stride_blocks(int64_t elements) {
  const int64_t blocks = (elements + 255) / 256;
  return static_cast<int>(blocks < 2048 ? blocks : 2048);
}

hipError_t panel_fill(int width, const double* base, int ncols, int kp, double* out,
                      hipStream_t s) {
  if (ncols <= 0) return hipSuccess;
  return for_panel_width(width, [&](auto w) {
    constexpr int K = decltype(w)::value;
    const int blocks = panel_stride_blocks(static_cast<int64_t>(ncols) * K);
    panel_fill_kernel<K><<<blocks, 256, 0, s>>>(base, ncols, kp, out);
  });
}

hipError_t panel_override(int width, const RowPanelOverrideArgs& args, int64_t num_overrides,
                          hipStream_t s) {
  if (num_overrides <= 0 || args.kp <= 0) return hipSuccess;
  const int blocks = panel_stride_blocks(num_overrides);
  return for_panel_width(width, [&](auto w) {
    panel_override_kernel<decltype(w)::value><<<blocks, 256, 0, s>>>(args);
  });
}

}  // namespace milp_launch
