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

// Rows deleted from the resident [A | I]: the compaction of the CSC and the
// CSR (DeviceLp::DeleteRows, kernel_args.h MatrixDeleteArgs). Only the mask
// comes from the host. Every position is a function of the input alone: a
// kept row's new index is the exclusive scan of the keep flags, its CSR start
// the scan of the kept rows' lengths, a column's new start the scan of its
// kept entries, and an entry's place in its column the kept entries before it.
// There is no atomic and no workgroup waits for another: each scan is a count
// pass per tile, one workgroup over the tile counts and a pass per tile again,
// as for the append above. Entry totals are int64 throughout.
namespace milp_kernels {

namespace {

// scan_block_exclusive (block_scan.h) for int64 values; lds_waves holds
// kDeleteThreads / kWave of them, and the same barrier rule applies.
__device__ __forceinline__ int64_t delete_scan64(int64_t c, int64_t* total, int64_t* lds_waves) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  long long x = c;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const long long y = __shfl_up(x, off, kWave);
    if (lane >= off) x += y;
  }
  if (lane == kWave - 1) lds_waves[wave] = x;
  __syncthreads();
  int64_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kDeleteThreads / kWave; ++w) {
    const int64_t v = lds_waves[w];
    before += w < wave ? v : 0;
    all += v;
  }
  *total = all;
  return before + x - c;
}

__device__ __forceinline__ bool delete_keeps(const MatrixDeleteArgs& a, int r) {
  return a.delete_mask[r] == 0;
}

}  // namespace

// row_tile_rows[tile] / row_tile_entries[tile] = the kept rows of the tile and
// their CSR entries.
__global__ __launch_bounds__(kDeleteTile) void delete_row_tile_count_kernel(MatrixDeleteArgs a) {
  __shared__ int lds_rows[kDeleteTile / kWave];
  __shared__ int64_t lds_entries[kDeleteTile / kWave];
  const int r = blockIdx.x * kDeleteTile + threadIdx.x;
  const bool keep = r < a.m && delete_keeps(a, r);
  const int64_t len = keep ? a.old_t_starts[r + 1] - a.old_t_starts[r] : 0;
  int rows;
  int64_t entries;
  (void)scan_block_exclusive<kDeleteTile>(keep ? 1 : 0, &rows, lds_rows);
  (void)delete_scan64(len, &entries, lds_entries);
  if (threadIdx.x == 0) {
    a.row_tile_rows[blockIdx.x] = rows;
    a.row_tile_entries[blockIdx.x] = entries;
  }
}

// Both tile arrays become exclusive prefixes, in place (a thread reads and
// writes its own tile only). One workgroup, the running totals in registers.
__global__ __launch_bounds__(kDeleteThreads) void delete_row_tile_offsets_kernel(
    MatrixDeleteArgs a) {
  __shared__ int lds_rows[kDeleteThreads / kWave];
  __shared__ int64_t lds_entries[kDeleteThreads / kWave];
  int running_rows = 0;
  int64_t running_entries = 0;
  for (int base = 0; base < a.row_tiles; base += kDeleteThreads) {
    const int tile = base + threadIdx.x;
    const int rows = tile < a.row_tiles ? a.row_tile_rows[tile] : 0;
    const int64_t entries = tile < a.row_tiles ? a.row_tile_entries[tile] : 0;
    int total_rows;
    int64_t total_entries;
    const int excl_rows = scan_block_exclusive<kDeleteThreads>(rows, &total_rows, lds_rows);
    const int64_t excl_entries = delete_scan64(entries, &total_entries, lds_entries);
    if (tile < a.row_tiles) {
      a.row_tile_rows[tile] = running_rows + excl_rows;
      a.row_tile_entries[tile] = running_entries + excl_entries;
    }
    running_rows += total_rows;
    running_entries += total_entries;
    __syncthreads();  // the next scans go through the same lds arrays
  }
}

// new_row[r] for every row, new_t_starts of the kept ones; the last row's
// thread closes the last kept row.
__global__ __launch_bounds__(kDeleteTile) void delete_row_map_kernel(MatrixDeleteArgs a) {
  __shared__ int lds_rows[kDeleteTile / kWave];
  __shared__ int64_t lds_entries[kDeleteTile / kWave];
  const int r = blockIdx.x * kDeleteTile + threadIdx.x;
  const bool keep = r < a.m && delete_keeps(a, r);
  const int64_t len = keep ? a.old_t_starts[r + 1] - a.old_t_starts[r] : 0;
  int rows;
  int64_t entries;
  const int at = a.row_tile_rows[blockIdx.x] +
                 scan_block_exclusive<kDeleteTile>(keep ? 1 : 0, &rows, lds_rows);
  const int64_t start = a.row_tile_entries[blockIdx.x] + delete_scan64(len, &entries, lds_entries);
  if (r >= a.m) return;
  a.new_row[r] = at;
  if (keep) a.new_t_starts[at] = start;
  if (r == a.m - 1) a.new_t_starts[at + (keep ? 1 : 0)] = start + len;
}

// Kept rows of at most kDeleteShort entries, one row per thread. A row's last
// entry is its slack: its column becomes n + the row's new index.
__global__ __launch_bounds__(kDeleteThreads) void delete_row_move_short_kernel(
    MatrixDeleteArgs a) {
  const int r = blockIdx.x * kDeleteThreads + threadIdx.x;
  if (r >= a.m || !delete_keeps(a, r)) return;
  const int64_t b = a.old_t_starts[r];
  const int64_t end = a.old_t_starts[r + 1];
  if (end - b > kDeleteShort) return;
  const int at = a.new_row[r];
  const int64_t shift = a.new_t_starts[at] - b;
  for (int64_t p = b; p < end; ++p) {
    a.new_t_cols[p + shift] = p == end - 1 ? a.n + at : a.old_t_cols[p];
    a.new_t_vals[p + shift] = a.old_t_vals[p];
  }
}

// The longer kept rows, one workgroup per row, consecutive threads on
// consecutive entries.
__global__ __launch_bounds__(kDeleteThreads) void delete_row_move_long_kernel(
    MatrixDeleteArgs a) {
  const int r = blockIdx.x;
  if (!delete_keeps(a, r)) return;
  const int64_t b = a.old_t_starts[r];
  const int64_t end = a.old_t_starts[r + 1];
  if (end - b <= kDeleteShort) return;
  const int at = a.new_row[r];
  const int64_t shift = a.new_t_starts[at] - b;
  for (int64_t p = b + threadIdx.x; p < end; p += kDeleteThreads) {
    a.new_t_cols[p + shift] = p == end - 1 ? a.n + at : a.old_t_cols[p];
    a.new_t_vals[p + shift] = a.old_t_vals[p];
  }
}

// count[c] = the entries of structural column c whose row is kept; the
// columns of at most kDeleteShort entries, one per thread.
__global__ __launch_bounds__(kDeleteThreads) void delete_col_count_short_kernel(
    MatrixDeleteArgs a) {
  const int c = blockIdx.x * kDeleteThreads + threadIdx.x;
  if (c >= a.n) return;
  const int64_t b = a.old_starts[c];
  const int64_t end = a.old_starts[c + 1];
  if (end - b > kDeleteShort) return;
  int kept = 0;
  for (int64_t p = b; p < end; ++p) kept += delete_keeps(a, a.old_rows[p]) ? 1 : 0;
  a.count[c] = kept;
}

// The longer columns, one workgroup each.
__global__ __launch_bounds__(kDeleteThreads) void delete_col_count_long_kernel(
    MatrixDeleteArgs a) {
  __shared__ int lds_waves[kDeleteThreads / kWave];
  const int c = blockIdx.x;
  const int64_t b = a.old_starts[c];
  const int64_t end = a.old_starts[c + 1];
  if (end - b <= kDeleteShort) return;
  int kept = 0;
  for (int64_t p = b + threadIdx.x; p < end; p += kDeleteThreads) {
    kept += delete_keeps(a, a.old_rows[p]) ? 1 : 0;
  }
  int total;
  (void)scan_block_exclusive<kDeleteThreads>(kept, &total, lds_waves);
  if (threadIdx.x == 0) a.count[c] = total;
}

// col_tile_entries[tile] = the kept entries of the tile's structural columns.
__global__ __launch_bounds__(kDeleteTile) void delete_col_tile_count_kernel(MatrixDeleteArgs a) {
  __shared__ int64_t lds_entries[kDeleteTile / kWave];
  const int c = blockIdx.x * kDeleteTile + threadIdx.x;
  int64_t total;
  (void)delete_scan64(c < a.n ? a.count[c] : 0, &total, lds_entries);
  if (threadIdx.x == 0) a.col_tile_entries[blockIdx.x] = total;
}

// col_tile_entries becomes its exclusive prefix, in place; one workgroup.
__global__ __launch_bounds__(kDeleteThreads) void delete_col_tile_offsets_kernel(
    MatrixDeleteArgs a) {
  __shared__ int64_t lds_entries[kDeleteThreads / kWave];
  int64_t running = 0;
  for (int base = 0; base < a.col_tiles; base += kDeleteThreads) {
    const int tile = base + threadIdx.x;
    const int64_t entries = tile < a.col_tiles ? a.col_tile_entries[tile] : 0;
    int64_t total;
    const int64_t excl = delete_scan64(entries, &total, lds_entries);
    if (tile < a.col_tiles) a.col_tile_entries[tile] = running + excl;
    running += total;
    __syncthreads();  // the next scan goes through the same lds_entries
  }
}

// new_starts[c] of the structural columns.
__global__ __launch_bounds__(kDeleteTile) void delete_col_starts_kernel(MatrixDeleteArgs a) {
  __shared__ int64_t lds_entries[kDeleteTile / kWave];
  const int c = blockIdx.x * kDeleteTile + threadIdx.x;
  int64_t total;
  const int64_t excl = delete_scan64(c < a.n ? a.count[c] : 0, &total, lds_entries);
  if (c < a.n) a.new_starts[c] = a.col_tile_entries[blockIdx.x] + excl;
}

// The columns of at most kDeleteShort entries: one thread walks its column
// and writes the kept entries in order, rows renumbered.
__global__ __launch_bounds__(kDeleteThreads) void delete_col_move_short_kernel(
    MatrixDeleteArgs a) {
  const int c = blockIdx.x * kDeleteThreads + threadIdx.x;
  if (c >= a.n) return;
  const int64_t b = a.old_starts[c];
  const int64_t end = a.old_starts[c + 1];
  if (end - b > kDeleteShort) return;
  int64_t out = a.new_starts[c];
  for (int64_t p = b; p < end; ++p) {
    const int r = a.old_rows[p];
    if (!delete_keeps(a, r)) continue;
    a.new_rows[out] = a.new_row[r];
    a.new_vals[out] = a.old_vals[p];
    ++out;
  }
}

// The longer columns, one workgroup each, in chunks of kDeleteThreads
// entries: the keep flags of a chunk are block-scanned, the kept entries
// before the chunk are a running base in a register (every thread computes
// the same one).
__global__ __launch_bounds__(kDeleteThreads) void delete_col_move_long_kernel(
    MatrixDeleteArgs a) {
  __shared__ int lds_waves[kDeleteThreads / kWave];
  const int c = blockIdx.x;
  const int64_t b = a.old_starts[c];
  const int64_t end = a.old_starts[c + 1];
  if (end - b <= kDeleteShort) return;
  int64_t base = a.new_starts[c];
  for (int64_t chunk = b; chunk < end; chunk += kDeleteThreads) {
    const int64_t p = chunk + threadIdx.x;
    const int r = p < end ? a.old_rows[p] : 0;
    const bool keep = p < end && delete_keeps(a, r);
    int total;
    const int excl = scan_block_exclusive<kDeleteThreads>(keep ? 1 : 0, &total, lds_waves);
    if (keep) {
      a.new_rows[base + excl] = a.new_row[r];
      a.new_vals[base + excl] = a.old_vals[p];
    }
    base += total;
    __syncthreads();  // the next scan goes through the same lds_waves
  }
}

// The slack columns, one thread per old row: kept slack j' is the one entry
// at new_structural + j' with the old slack's value bits; thread m closes the
// last column.
__global__ __launch_bounds__(kDeleteThreads) void delete_slacks_kernel(MatrixDeleteArgs a) {
  const int i = blockIdx.x * kDeleteThreads + threadIdx.x;
  if (i > a.m) return;
  if (i == a.m) {
    a.new_starts[a.n + a.kept] = a.new_structural + a.kept;
    return;
  }
  if (!delete_keeps(a, i)) return;
  const int at = a.new_row[i];
  const int64_t to = a.new_structural + at;
  a.new_starts[a.n + at] = to;
  a.new_rows[to] = at;
  a.new_vals[to] = a.old_vals[a.old_starts[a.n + i]];
}

}  // namespace milp_kernels

namespace milp_launch {

hipError_t matrix_delete_rows(const milp_kernels::MatrixDeleteArgs& args, bool long_columns,
                              bool long_rows, hipStream_t s) {
  using namespace milp_kernels;
  if (args.n < 0 || args.m <= 0 || args.kept <= 0 || args.kept > args.m ||
      args.new_structural < 0 || args.row_tiles != (args.m + kDeleteTile - 1) / kDeleteTile ||
      args.col_tiles != (args.n + kDeleteTile - 1) / kDeleteTile) {
    return hipErrorInvalidValue;
  }
  const int row_blocks = (args.m + kDeleteThreads - 1) / kDeleteThreads;
  delete_row_tile_count_kernel<<<args.row_tiles, kDeleteTile, 0, s>>>(args);
  delete_row_tile_offsets_kernel<<<1, kDeleteThreads, 0, s>>>(args);
  delete_row_map_kernel<<<args.row_tiles, kDeleteTile, 0, s>>>(args);
  delete_row_move_short_kernel<<<row_blocks, kDeleteThreads, 0, s>>>(args);
  if (long_rows) delete_row_move_long_kernel<<<args.m, kDeleteThreads, 0, s>>>(args);
  if (args.n > 0) {
    const int col_blocks = (args.n + kDeleteThreads - 1) / kDeleteThreads;
    delete_col_count_short_kernel<<<col_blocks, kDeleteThreads, 0, s>>>(args);
    if (long_columns) delete_col_count_long_kernel<<<args.n, kDeleteThreads, 0, s>>>(args);
    delete_col_tile_count_kernel<<<args.col_tiles, kDeleteTile, 0, s>>>(args);
    delete_col_tile_offsets_kernel<<<1, kDeleteThreads, 0, s>>>(args);
    delete_col_starts_kernel<<<args.col_tiles, kDeleteTile, 0, s>>>(args);
    delete_col_move_short_kernel<<<col_blocks, kDeleteThreads, 0, s>>>(args);
    if (long_columns) delete_col_move_long_kernel<<<args.n, kDeleteThreads, 0, s>>>(args);
  }
  delete_slacks_kernel<<<(args.m + 1 + kDeleteThreads - 1) / kDeleteThreads, kDeleteThreads, 0,
                         s>>>(args);
  return hipGetLastError();
}

}  // namespace milp_launch
