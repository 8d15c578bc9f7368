// Rows appended to the resident [A | I]: the merge of k new rows into the CSC
// (DeviceLp::AppendRows, kernel_args.h MatrixAppendArgs). The new rows are
// read from the tail of the new CSR, which is all that crosses PCIe; the old
// CSC never leaves the device.
//
// Every position is a function of the input alone: an entry (row j, column c)
// goes to new_starts[c + 1] - add[c] + rank, rank = the rows j' < j that hold
// c, so that a column's new entries land in ascending row order. The only
// atomic is the integer count add[c]; no position comes from its return value.
// No workgroup waits for another: the offsets are a count pass per tile, one
// workgroup over the tile counts, and a pass per tile again (the scheme of
// panel_count / panel_offsets / panel_write).
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "kernel_args.h"

namespace milp_kernels {

namespace {

// The new row of the tail entry at absolute CSR position `at`: the largest j
// with tail_starts[j] <= at (rows may be empty but for their slack, so the
// starts strictly increase).
__device__ __forceinline__ int append_row_of(const int64_t* __restrict__ tail_starts, int k,
                                             int64_t at) {
  int lo = 0, hi = k;  // tail_starts[lo] <= at < tail_starts[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tail_starts[mid] <= at) lo = mid; else hi = mid;
  }
  return lo;
}

// Whether the ascending columns t_cols[b, e) hold c.
__device__ __forceinline__ bool append_holds(const int32_t* __restrict__ t_cols, int64_t b,
                                             int64_t e, int32_t c) {
  while (b < e) {
    const int64_t mid = (b + e) >> 1;
    const int32_t v = t_cols[mid];
    if (v == c) return true;
    if (v < c) b = mid + 1; else e = mid;
  }
  return false;
}

}  // namespace

// One thread per tail entry: rank[q] and add[c] of a structural entry (a
// row's last entry is its slack and has neither).
__global__ __launch_bounds__(kAppendThreads) void append_rank_count_kernel(MatrixAppendArgs a) {
  const int64_t q = static_cast<int64_t>(blockIdx.x) * kAppendThreads + threadIdx.x;
  if (q >= a.e + a.k) return;
  const int64_t at = a.tail_starts[0] + q;
  const int j = append_row_of(a.tail_starts, a.k, at);
  if (at == a.tail_starts[j + 1] - 1) return;  // the slack
  const int32_t c = a.t_cols[at];
  int r = 0;
  for (int jj = 0; jj < j; ++jj) {
    r += append_holds(a.t_cols, a.tail_starts[jj], a.tail_starts[jj + 1] - 1, c) ? 1 : 0;
  }
  a.rank[q] = r;
  atomicAdd(&a.add[c], 1);
}

// tile_counts[tile] = the new entries of the tile's structural columns.
__global__ __launch_bounds__(kAppendTileColumns) void append_tile_count_kernel(
    MatrixAppendArgs a) {
  __shared__ int lds_waves[kAppendTileColumns / kWave];
  const int c = blockIdx.x * kAppendTileColumns + threadIdx.x;
  int total;
  (void)scan_block_exclusive<kAppendTileColumns>(c < a.n ? a.add[c] : 0, &total, lds_waves);
  if (threadIdx.x == 0) a.tile_counts[blockIdx.x] = total;
}

// tile_offsets[tile] = the new entries of the tiles before it. One workgroup,
// a block scan per step of kAppendThreads tiles, the running total in a
// register (every thread computes the same one).
__global__ __launch_bounds__(kAppendThreads) void append_tile_offsets_kernel(MatrixAppendArgs a) {
  __shared__ int lds_waves[kAppendThreads / kWave];
  int64_t running = 0;
  for (int base = 0; base < a.tiles; base += kAppendThreads) {
    const int tile = base + threadIdx.x;
    const int c = tile < a.tiles ? a.tile_counts[tile] : 0;
    int total;
    const int excl = scan_block_exclusive<kAppendThreads>(c, &total, lds_waves);
    if (tile < a.tiles) a.tile_offsets[tile] = running + excl;
    running += total;
    __syncthreads();  // the next scan goes through the same lds_waves
  }
}

// new_starts[c] = old_starts[c] + the new entries of the columns before c,
// for the structural columns.
__global__ __launch_bounds__(kAppendTileColumns) void append_starts_kernel(MatrixAppendArgs a) {
  __shared__ int lds_waves[kAppendTileColumns / kWave];
  const int c = blockIdx.x * kAppendTileColumns + threadIdx.x;
  int total;
  const int excl =
      scan_block_exclusive<kAppendTileColumns>(c < a.n ? a.add[c] : 0, &total, lds_waves);
  if (c < a.n) a.new_starts[c] = a.old_starts[c] + a.tile_offsets[blockIdx.x] + excl;
}

// The slack columns, one thread each: old slack i moves back by e, new slack
// j starts at nnz + e + j (its entry is written by append_scatter_kernel), and
// i = m + k closes the last column.
__global__ __launch_bounds__(kAppendThreads) void append_slacks_kernel(MatrixAppendArgs a) {
  const int i = blockIdx.x * kAppendThreads + threadIdx.x;
  if (i > a.m + a.k) return;
  if (i >= a.m) {
    a.new_starts[a.n + i] = a.nnz + a.e + (i - a.m);
    return;
  }
  const int64_t b = a.old_starts[a.n + i];
  const int64_t end = a.old_starts[a.n + i + 1];
  a.new_starts[a.n + i] = b + a.e;
  for (int64_t p = b; p < end; ++p) {
    a.new_rows[p + a.e] = a.old_rows[p];
    a.new_vals[p + a.e] = a.old_vals[p];
  }
}

// Old entries of the structural columns of at most kAppendShortColumn
// entries, one column per thread (neighbouring threads copy neighbouring
// ranges).
__global__ __launch_bounds__(kAppendThreads) void append_move_short_kernel(MatrixAppendArgs a) {
  const int c = blockIdx.x * kAppendThreads + threadIdx.x;
  if (c >= a.n) return;
  const int64_t b = a.old_starts[c];
  const int64_t end = a.old_starts[c + 1];
  if (end - b > kAppendShortColumn) return;
  const int64_t shift = a.new_starts[c] - b;
  for (int64_t p = b; p < end; ++p) {
    a.new_rows[p + shift] = a.old_rows[p];
    a.new_vals[p + shift] = a.old_vals[p];
  }
}

// The longer columns, one workgroup per column: consecutive threads move
// consecutive entries (coalesced 4- and 8-byte accesses).
__global__ __launch_bounds__(kAppendThreads) void append_move_long_kernel(MatrixAppendArgs a) {
  const int c = blockIdx.x;
  const int64_t b = a.old_starts[c];
  const int64_t end = a.old_starts[c + 1];
  if (end - b <= kAppendShortColumn) return;
  const int64_t shift = a.new_starts[c] - b;
  for (int64_t p = b + threadIdx.x; p < end; p += kAppendThreads) {
    a.new_rows[p + shift] = a.old_rows[p];
    a.new_vals[p + shift] = a.old_vals[p];
  }
}

// One thread per tail entry again, after the starts: the entry goes to its
// column's end, the row's slack entry to the new slack column.
__global__ __launch_bounds__(kAppendThreads) void append_scatter_kernel(MatrixAppendArgs a) {
  const int64_t q = static_cast<int64_t>(blockIdx.x) * kAppendThreads + threadIdx.x;
  if (q >= a.e + a.k) return;
  const int64_t at = a.tail_starts[0] + q;
  const int j = append_row_of(a.tail_starts, a.k, at);
  int64_t to;
  if (at == a.tail_starts[j + 1] - 1) {
    to = a.nnz + a.e + j;
  } else {
    const int32_t c = a.t_cols[at];
    to = a.new_starts[c + 1] - a.add[c] + a.rank[q];
  }
  a.new_rows[to] = a.m + j;
  a.new_vals[to] = a.t_vals[at];
}

}  // namespace milp_kernels

namespace milp_launch {

hipError_t matrix_append_rows(const milp_kernels::MatrixAppendArgs& args, bool long_columns,
                              hipStream_t s) {
  using namespace milp_kernels;
  if (args.n < 0 || args.m < 0 || args.k < 0 || args.e < 0 ||
      args.tiles != (args.n + kAppendTileColumns - 1) / kAppendTileColumns) {
    return hipErrorInvalidValue;
  }
  const int64_t tail = args.e + args.k;
  const unsigned tail_blocks = static_cast<unsigned>((tail + kAppendThreads - 1) / kAppendThreads);
  if (tail > 0) append_rank_count_kernel<<<tail_blocks, kAppendThreads, 0, s>>>(args);
  if (args.tiles > 0) {
    append_tile_count_kernel<<<args.tiles, kAppendTileColumns, 0, s>>>(args);
    append_tile_offsets_kernel<<<1, kAppendThreads, 0, s>>>(args);
    append_starts_kernel<<<args.tiles, kAppendTileColumns, 0, s>>>(args);
  }
  const int slack_threads = args.m + args.k + 1;
  append_slacks_kernel<<<(slack_threads + kAppendThreads - 1) / kAppendThreads, kAppendThreads, 0,
                         s>>>(args);
  if (args.n > 0) {
    append_move_short_kernel<<<(args.n + kAppendThreads - 1) / kAppendThreads, kAppendThreads, 0,
                               s>>>(args);
    if (long_columns) append_move_long_kernel<<<args.n, kAppendThreads, 0, s>>>(args);
  }
  if (tail > 0) append_scatter_kernel<<<tail_blocks, kAppendThreads, 0, s>>>(args);
  return hipGetLastError();
}

}  // namespace milp_launch
