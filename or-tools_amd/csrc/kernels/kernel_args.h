// Argument blocks shared by the kernel launchers (simplex_kernels.hip) and
// the device layer (engine/device_lp.hip). Plain structs of device pointers.
#ifndef MILP_KERNEL_ARGS_H_
#define MILP_KERNEL_ARGS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace milp_kernels {

struct DotArgs {
  const int64_t* starts;
  const int32_t* rows;
  const double* vals;
  const double* y;
  int ncols;                // columns to visit (N, or list length)
  const int32_t* col_list;  // kListDots: the columns
  const uint64_t* mask;     // relevance / not-basic bitset (modes 0, 3)
  const double* c;          // kPricing: objective + perturbation
  double* out;              // result per column (or per list entry)
  uint8_t* flags;           // kUpdateRowColumnWise: |coeff| > drop; kListDots: listed
  double drop_tolerance;
  const uint8_t* skip;      // optional: columns handled by the dense block
  const double* y2;         // kUpdateRowWithDots / kPricingWithDots: w = B^-T d
  double* out2;             // w . a_j for listed columns
};

// Dense column block: the structural columns whose CSC column is full (all m
// rows). Values only, chain-major so that lane j of the wave for chain k
// streams chain k of column j (Glop's accumulator r_{k+1} in
// ColumnScalarProduct, sparse.h:514-542, since a full column's entry index
// equals its row index) with 16-byte loads that are contiguous across the
// wave. With steps = m / 4 chain elements per chain and pairs = steps / 2:
//   body[((t2 * 4 + k) * nd + j) * 2 + h] = A[4 (2 t2 + h) + k, col_j], t2 < pairs
//   body[pairs * nd * 8 + k * nd + j]     = A[4 (steps - 1) + k, col_j] if steps odd
//   tail[r * nd + j]                      = A[4 steps + r, col_j],       r < m % 4
struct DenseArgs {
  const double* body;
  const double* tail;
  const int32_t* dense_cols;  // nd ascending column ids
  int nd;
  int m;
  const double* y;        // dot vector (rho / y / w)
  const uint64_t* mask;   // kUpdateRowColumnWise: relevant columns
  const double* c;        // kPricing
  double* out;            // indexed by column id
  uint8_t* flags;         // kUpdateRowColumnWise: out; kListDots: in (listed)
  double drop_tolerance;
  const double* y2;       // kUpdateRowWithDots / kPricingWithDots
  double* out2;
};

// Column dots against a panel of K vectors (panel_kernels.hip). The vectors
// are row-interleaved, y[r * K + v], zero for the padding vectors v >= kp;
// the results are column-interleaved, out[col * K + v], written for v < kp.
constexpr int kPanelMaxWidth = 16;  // the widths are 1, 4 and 16
struct PanelDotArgs {
  const int64_t* starts;  // CSC of [A | I]
  const int32_t* rows;
  const double* vals;
  const double* y;
  int ncols;                // columns to visit (N, or list length)
  const int32_t* col_list;  // the columns, or nullptr for 0 .. ncols - 1
  int kp;                   // vectors in use (<= K)
  double* out;
};
struct PanelDenseArgs {  // the dense block of DenseArgs
  const double* body;
  const double* tail;
  const int32_t* dense_cols;
  int nd;
  int m;
  const double* y;
  int kp;
  double* out;
};

// The panel result filtered and packed into sparse rows (panel_kernels.hip,
// panel_count / panel_offsets / panel_write). Entry (col, v) is kept when
// the column's mask bit is set (mask == nullptr: every column) and
// fabs(in[col * K + v]) > drop_tolerance. Vector v's kept entries, columns
// ascending, start at the sum of totals[0 .. v) in cols / vals.
constexpr int kPanelTileColumns = 256;  // columns of one workgroup's tile
constexpr int kPanelOffsetsStep = 256;  // tiles per block scan of panel_offsets
struct PanelSparseArgs {
  const double* in;      // interleaved panel result, ncols x K
  int ncols;
  int kp;                // vectors in use (<= K)
  int tiles;             // ceil(ncols / kPanelTileColumns)
  const uint64_t* mask;  // ceil(ncols / 64) words, or nullptr
  double drop_tolerance;
  int* counts;           // kp x tiles
  int64_t* offsets;      // kp x tiles
  int64_t* totals;       // kp
  int32_t* cols;         // packed output; room for ncols * kp entries
  double* vals;
};

// The panel result reduced to one branching penalty record per vector
// (panel_kernels.hip, penalties_tile / penalties_fold; include/mi_lp.h
// mi_lp_row_penalties has the rule). alpha = in[col * K + v]; d, status and
// unit are per column, dist per vector. A column that takes part in a
// direction adds one to its count and offers a candidate >= +0.0 (never NaN,
// never -0.0); the record keeps the smallest candidate and the lowest column
// attaining it. Partials are (minimum, column, count) per (vector, direction,
// tile), at [(v * 2 + direction) * tiles + tile], direction 0 = down; without
// a column they are (+inf, kNoPenaltyColumn, 0).
struct BranchPenalty {  // mi_lp_branch_penalty of include/mi_lp.h
  double down;
  double up;
  int32_t down_col;
  int32_t up_col;
  int32_t down_count;
  int32_t up_count;
};
constexpr int kNoPenaltyColumn = 0x7fffffff;
struct PenaltyArgs {
  const double* in;       // interleaved panel result, ncols x K
  int ncols;
  int kp;                 // vectors in use (<= K)
  int tiles;              // ceil(ncols / kPanelTileColumns)
  const double* d;        // ncols: reduced costs, minimisation sense
  const uint8_t* status;  // ncols: MI_LP_BASIC .. MI_LP_FREE
  const double* unit;     // ncols: integer steps, or nullptr (all 0)
  const double* down_dist;  // kp: the panel's vectors
  const double* up_dist;    // kp
  double pivot_tolerance;
  double* tile_min;       // 2 kp x tiles
  int32_t* tile_col;      // 2 kp x tiles
  int* tile_count;        // 2 kp x tiles
  BranchPenalty* out;     // kp
};

// The panel result turned into Gomory mixed-integer cuts in the structural
// space (panel_kernels.hip, gomory_transform_tile / gomory_combine_tile /
// gomory_fold; include/mi_lp.h mi_lp_row_gomory_cuts has the rule). All three
// interleaved arrays share one layout, [col * K + v].
//   transform  alpha = cols[col * K + v] over all ncols columns -> g: the
//              structural part to g[col * K + v] (col < n), the slack part to
//              slack[(col - n) * K + v], which is the row-interleaved vector
//              y' of the second dot pass; bad-column counts per (vector, tile)
//              at tile_bad[v * tiles + tile].
//   combine    s = cols[col * K + v] of the second pass over the n structural
//              columns -> c = g - s written back to cols; per (vector, tile)
//              at [v * tiles_n + tile] the kept count, the NaN count, the
//              largest and the smallest fabs(c) among the kept entries and
//              the lowest column attaining each. Without a kept entry the
//              partials are (0.0, kNoCutColumn) and (+inf, kNoCutColumn): a
//              kept entry has fabs(c) > 0, and a kept +inf sits at a real
//              column.
//   fold       workgroup v: one CutSummary.
struct CutSummary {  // mi_lp_cut_summary of include/mi_lp.h
  double max_abs;
  double min_abs;
  int32_t count;
  int32_t bad_count;
  int32_t max_col;
  int32_t min_col;
};
constexpr int kNoCutColumn = 0x7fffffff;
struct GomoryArgs {
  double* cols;           // interleaved panel result, ncols x K (c overwrites s for col < n)
  double* g;              // max(1, n) x K
  double* slack;          // max(1, m) x K: the dot kernels' y
  int ncols;              // n + m
  int n;                  // structural columns
  int kp;                 // vectors in use (<= K)
  int tiles;              // ceil(ncols / kPanelTileColumns)
  int tiles_n;            // ceil(n / kPanelTileColumns)
  const uint8_t* status;  // ncols: MI_LP_BASIC .. MI_LP_FREE
  const double* unit;     // ncols: integer steps, or nullptr (all 0)
  const double* f0;        // kp: the panel's vectors
  const double* row_unit;  // kp
  double zero_tolerance;
  double drop_tolerance;
  int* tile_bad;           // kp x tiles
  int* tile_count;         // kp x tiles_n
  int* tile_nan;           // kp x tiles_n
  double* tile_max;        // kp x tiles_n
  double* tile_min;        // kp x tiles_n
  int32_t* tile_max_col;   // kp x tiles_n
  int32_t* tile_min_col;   // kp x tiles_n
  CutSummary* out;         // kp
};

// Row sums of [A | I] against a panel of K points (panel_kernels.hip,
// row_sums_panel). The points are column-interleaved, x[col * K + v], zero
// for the padding points v >= kp; the results are row-interleaved,
// out[row * K + v], written for v < kp. A 256-thread workgroup owns 256 / K
// rows; the kernel reads the rows' entries directly (no LDS staging).
constexpr int kRowPanelThreads = 256;
constexpr int kRowPanelUnroll = 8;  // x gathers in flight ahead of the ordered adds
constexpr int kRowPanelChunk = 0;   // staging chunk length; 0: the kernel does not stage
struct RowPanelArgs {
  const int64_t* t_starts;  // CSR of [A | I]
  const int32_t* t_cols;
  const double* t_vals;
  const double* x;
  int num_rows;
  int kp;  // points in use (<= K)
  double* out;
};
// The overrides of one panel scattered into the interleaved points:
// x[cols[i] * K + v] = vals[i] for i in [starts[v], starts[v + 1]), v < kp.
// No column repeats within a point, so no two stores meet.
struct RowPanelOverrideArgs {
  const int64_t* starts;  // kp + 1 entries, positions into cols / vals
  const int32_t* cols;
  const double* vals;
  int kp;
  double* x;
};

// The violated rows of the row-sum panel result and one summary per point
// (panel_kernels.hip, violations_count / panel_offsets / violations_fold /
// violations_write; include/mi_lp.h mi_lp_column_combinations_violations).
// Row r is violated at point v when a = in[r * K + v] has
// !(a >= row_lb[r] - tolerance) || !(a <= row_ub[r] + tolerance); both
// widened bounds are formed in the kernels, one rounded operation each. Its
// amount is +inf for a NaN a, else max(row_lb[r] - a, a - row_ub[r]).
// Point v's violated rows, ascending, start at the sum of totals[0 .. v) in
// rows / activities. The tiles are kPanelTileColumns consecutive rows.
struct PointViolations {  // mi_lp_point_violations of include/mi_lp.h
  int64_t count;
  double worst;
  int32_t worst_row;
  int32_t reserved;
};
//
// The same passes serve the bound sets' screening (activity_ranges_panel
// below) under the second rule: `in` then holds g per (row, child), row r
// proves child v infeasible when g > tolerance, and its amount is g (> 0,
// never NaN). row_lb / row_ub are not read under that rule.
//
// The third rule serves the implied column bounds (implied_bounds_panel
// below): `in` holds one key per (column, child), num_rows is the number of
// columns, a key >= 0 is kept and a key > 0 is a crossing column with that
// amount. A kept column that does not cross enters the worst-merge without an
// index, so a summary has count > 0 and worst_row == -1 when no column
// crosses. row_lb / row_ub / tolerance are not read under that rule.
enum PanelRowRule { kRowRuleOutsideBounds = 0, kRowRuleAboveTolerance = 1, kRowRuleKeptKey = 2 };
struct RowViolationArgs {
  const double* in;      // interleaved row sums (or g), num_rows x K
  int num_rows;
  int kp;                // points in use (<= K)
  int tiles;             // ceil(num_rows / kPanelTileColumns)
  const double* row_lb;  // num_rows (kRowRuleOutsideBounds)
  const double* row_ub;
  double tolerance;
  int* counts;           // kp x tiles
  double* tile_worst;    // kp x tiles: the largest amount of (point, tile), 0.0 without one
  int32_t* tile_worst_row;  // kp x tiles: the lowest row attaining it
  int64_t* offsets;      // kp x tiles
  int64_t* totals;       // kp
  PointViolations* summaries;  // kp, or nullptr: no fold
  int32_t* rows;         // packed output, or nullptr: no offsets and no write pass
  double* activities;
};

// Activity ranges of the rows of A under a panel of K bound sets
// (panel_kernels.hip, activity_ranges_panel; include/mi_lp.h
// mi_lp_bound_activity_ranges has the rule). The bounds are two
// column-interleaved arrays over the num_structural columns,
// lower[col * K + v] and upper[col * K + v], 0.0 for the padding children
// v >= kp; entries of a CSR row with col >= num_structural (the slack) are
// skipped. Per (row, child) two sums from +0.0 in increasing column order and
// two counts of infinite bounds. Both arrays hold at least one element.
//   row_lb == nullptr  out receives three row-interleaved blocks of
//                      num_rows x K 8-byte words: lo, hi, and the counts
//                      packed as lo_inf | hi_inf << 32.
//   row_lb != nullptr  out receives g per (row, child) only: num_rows x K
//                      (the input of the kRowRuleAboveTolerance passes).
struct ActivityRangeArgs {
  const int64_t* t_starts;  // CSR of [A | I]
  const int32_t* t_cols;
  const double* t_vals;
  const double* lower;
  const double* upper;
  int num_rows;
  int num_structural;
  int kp;                // children in use (<= K)
  const double* row_lb;  // num_rows each, or both nullptr
  const double* row_ub;
  double* out;
};

// Implied column bounds of a panel of K bound sets (panel_kernels.hip,
// implied_bounds_panel; include/mi_lp.h mi_lp_bound_implied_bounds has the
// rule): the column direction over activity_ranges_panel's dense result.
// `ranges` is that kernel's `out` (row_lb == nullptr): lo, hi and the packed
// counts, three row-interleaved blocks of num_rows x K. lower / upper are the
// column-interleaved own bounds that kernel read. The CSC covers the
// num_cols structural columns (rows < num_rows). Results are
// column-interleaved, new_lower[col * K + v] and new_upper[col * K + v],
// written for v < kp.
//   keys != nullptr  also one key per (column, child), keys[col * K + v]:
//                    -1.0 for a column that is not kept, the crossing amount
//                    nl - nu (> tolerance >= 0) for a crossing column, else
//                    0.0. The kRowRuleKeptKey passes (below) filter them.
//   base_lb != nullptr  the override form: a column whose own bounds differ in
//                    bits from base_lb[col] / base_ub[col] is kept too.
struct ImpliedBoundsArgs {
  const int64_t* starts;  // CSC, num_cols + 1
  const int32_t* rows;
  const double* vals;
  const double* ranges;
  const double* row_lb;  // num_rows each
  const double* row_ub;
  const double* lower;
  const double* upper;
  int num_rows;
  int num_cols;
  int kp;  // children in use (<= K)
  double tolerance;
  const double* base_lb;  // num_cols each, or both nullptr
  const double* base_ub;
  double* new_lower;
  double* new_upper;
  double* keys;
};
// new_lower / new_upper at the kept columns of the kRowRuleKeptKey write pass:
// child v's kept columns are cols[sum of totals[0 .. v) ...], and
// out_lower / out_upper receive the two bounds at the same positions.
struct ImpliedGatherArgs {
  const int64_t* totals;  // kp
  const int32_t* cols;
  const double* new_lower;  // column-interleaved, num_cols x K
  const double* new_upper;
  int num_cols;
  int kp;
  double* out_lower;
  double* out_upper;
};

// One round of bound propagation applied to a panel of K bound sets
// (panel_kernels.hip, propagate_apply; include/mi_lp.h mi_lp_bound_propagate
// has the rule). new_lower / new_upper are implied_bounds_panel's results of
// this round, lower / upper the column-interleaved own bounds it read; every
// (column, set) with v < kp is one thread's:
//   integer columns round nl up and nu down (integrality_tolerance);
//   moved columns take (nl, nu) into lower / upper IN PLACE, others keep both;
//   keys[col * K + v] is -1.0 for a column that neither moved nor crosses, the
//   crossing amount l' - u' (> tolerance >= 0) for a crossing one, else 0.0:
//   the input of the kRowRuleKeptKey passes.
//   moved_keys != nullptr  also 0.0 for a moved column and -1.0 for any other
//                    (a column that crosses without a move is no move).
// Bit v of `frozen` is a set that has stopped: its lanes write -1.0 keys and
// leave the bounds alone.
struct PropagateApplyArgs {
  const double* new_lower;  // column-interleaved, num_cols x K
  const double* new_upper;
  double* lower;
  double* upper;
  const uint8_t* is_integer;  // num_cols, or nullptr: no integer column
  int num_cols;
  int kp;  // sets in use (<= K)
  double tolerance;
  double integrality_tolerance;
  uint32_t frozen;
  double* keys;
  double* moved_keys;
};
// The keys of the propagated lists: per (column, set) -1.0 for a column whose
// bounds equal base_lb[col] / base_ub[col] in bits and do not cross, the
// crossing amount lower - upper (> tolerance) for a crossing one, else 0.0.
struct PropagateChangedArgs {
  const double* lower;  // column-interleaved, num_cols x K
  const double* upper;
  const double* base_lb;  // num_cols each
  const double* base_ub;
  int num_cols;
  int kp;
  double tolerance;
  double* keys;
};

// Where an update-row kernel that emits the list itself puts it: the
// ascending listed columns, their coefficients and the count, on the device
// and (optional, null when off) mirrored into mapped host memory.
struct ListOut {
  int32_t* list;
  double* vals;
  int* count;
  int32_t* host_list;
  double* host_vals;
  int* host_count;
};

struct RowWiseArgs {
  const int64_t* t_starts;  // CSR of [A | I] (transposed_matrix_)
  const int32_t* t_cols;
  const double* t_vals;
  const int32_t* filtered_rows;  // list order (ascending for the chunk and list kernels)
  const double* rho;             // rho value per filtered row
  int num_filtered;
  int num_cols;
  const uint64_t* relevant;
  double* coefficient;  // update row (device copy of UpdateRow::coefficient_)
  uint8_t* flags;       // listed positions
  double drop_tolerance;
  int algorithm;  // 0 single row, 1 hypersparse, 2 row-wise
};

// The hypersparse update row of a large LP straight to its list, one
// workgroup (row_wise_list_kernel): algorithm 0 or 1, at most kListRowsMax
// filtered rows holding at most kListEntriesMax entries together (checked by
// the host). No flags and no N-sized pass (flags and num_cols are ignored;
// coefficient is scattered: touched (algorithm 1) / listed (0) columns): the
// entries are merged by column in LDS (12 B per entry + 2 B of permutation:
// 56 KB at the cap).
constexpr int kListEntriesMax = 4096;
constexpr int kListRowsMax = 64;
struct RowWiseListArgs : RowWiseArgs {
  ListOut out;
};

// The whole row-wise update row of a small LP in ONE workgroup and one launch
// (row_wise_small_kernel): N <= kSmallLdsCols, 1 <= filtered rows <=
// kSmallRowsMax, their entries <= kSmallEntries (checked by the host). The
// filtered rows, their rho values and the relevant mask are read from mapped
// host memory; the list lands in mapped host memory (and the device copies).
constexpr int kSmallLdsCols = 8192;
// The column-wise update row of a small LP without a dense block (m <=
// kSmallColWiseRows) in one workgroup: rho (and w) staged from mapped host
// memory into LDS, one thread per relevant column in ColumnScalarProduct's chain
// order, column_dot_kernel's kUpdateRowColumnWise / kUpdateRowWithDots write
// rules, then the compaction; list, values (and the w dots, list order) land
// in mapped host memory.
constexpr int kSmallColWiseRows = 4096;
struct ColWiseSmallArgs {
  const int64_t* starts;
  const int32_t* rows;
  const double* vals;
  const double* rho;       // mapped host memory, m values
  const double* w;         // mapped host memory, m values, or nullptr
  int m;
  int num_cols;            // <= kSmallLdsCols
  const uint64_t* relevant;  // mapped host memory
  double* coefficient;
  uint8_t* flags;
  double* out2;            // w . a_j of kept columns (device, per column)
  double drop_tolerance;
  ListOut out;
  double* host_dots;   // mapped host memory, list order (with w)
};

// The row-wise update row of a small LP with many filtered rows (or rows too
// long for kSmallEntries), one workgroup: thread per column over the CSC copy
// (row_wise_by_column_kernel's per-column order), row positions in LDS, then
// the compaction. m, N <= kSmallLdsCols; filtered rows <= m.
struct RowWiseSmallColArgs {
  const int64_t* starts;  // CSC of [A | I]
  const int32_t* rows;
  const double* vals;
  const int32_t* filtered_rows;  // mapped host memory, list order
  const double* rho;             // mapped host memory, rho per filtered row
  int num_filtered;
  int m;
  int num_cols;
  const uint64_t* relevant;      // mapped host memory
  double* coefficient;
  uint8_t* flags;
  double drop_tolerance;
  int algorithm;
  ListOut out;
};

// out[k] = a_{list[k]} . y for a small LP without a dense block, one
// workgroup: y (m <= kSmallLdsCols) staged from mapped host memory into LDS,
// one thread per column in ColumnScalarProduct's chain order, the results
// written straight to mapped host memory.
struct ListDotsSmallArgs {
  const int64_t* starts;
  const int32_t* rows;
  const double* vals;
  const double* y;  // mapped host memory, m values
  int m;
  const int32_t* list;  // device: compacted update-row list
  int n;
  double* out;  // mapped host memory
};
constexpr int kSmallRowsMax = 1024;
constexpr int kSmallEntries = 4096;
// RowWiseArgs with filtered_rows (list order), rho and relevant in mapped
// host memory, plus the list output.
using RowWiseSmallArgs = RowWiseListArgs;
constexpr int kMediumCols = 65536;

// The row-wise update row when every filtered row is full (all structural
// columns present): entry j < num_structural of CSR row r is column j and the
// row's last entry is its slack column. Slack outputs use the row tags.
struct RowWiseFullArgs {
  const int64_t* t_starts;  // CSR of [A | I]
  const double* t_vals;
  const int64_t* row_offsets;  // t_starts of each filtered row, list order k
  const double* rho;           // rho value per filtered row
  int num_filtered;
  int num_structural;
  int num_cols;
  const uint32_t* row_tag;
  const int32_t* row_pos;
  uint32_t tag;
  const uint64_t* relevant;
  double* coefficient;
  uint8_t* flags;
  double drop_tolerance;
  int algorithm;
};

// The same row-wise update row evaluated column by column from the CSC copy
// (for many filtered rows): row r of the filtered list sits at position
// row_pos[r] when row_tag[r] == tag.
struct RowWiseColArgs {
  const int64_t* starts;  // CSC of [A | I]
  const int32_t* rows;
  const double* vals;
  const uint32_t* row_tag;
  const int32_t* row_pos;
  uint32_t tag;
  const double* rho;  // rho value per filtered row, list order
  int num_cols;
  const uint64_t* relevant;
  double* coefficient;
  uint8_t* flags;
  double drop_tolerance;
  int algorithm;  // 0 single row, 1 hypersparse, 2 row-wise
};

// Dual simplex with device-resident reduced costs (engine/device_lp.h
// "dual device mode"). Per column one status byte:
//   bit 0 can_decrease, bit 1 can_increase, bit 2 non-basic boxed,
//   bits 3-5 glop::VariableStatus.
enum : uint8_t { kColCanDecrease = 1, kColCanIncrease = 2, kColBoxed = 4 };
__host__ __device__ inline int ColStatus(uint8_t b) { return (b >> 3) & 7; }

// Bound-flipping ratio test filter (entering_variable.cc:37-130) over the
// update-row list: pass 1 bounds the breakpoints that can matter, pass 2
// flags them.
struct DualRatioArgs {
  const int32_t* list;       // update-row positions (list order)
  const double* list_coeff;  // their coefficients
  const int* count;          // list length (device)
  int max_count;             // host-known bound of *count (sizes the grids)
  const double* rc;
  const uint8_t* colbits;
  const double* bound_diff;  // upper - lower per column
  double sign;               // +1 if cost_variation > 0 else -1
  double threshold;          // minimum pivot magnitude
  double harris_tolerance;
  double minimum_delta;
  double variation_magnitude;
  unsigned long long* best;  // pass 1: min over H-setting breakpoints of the
                             // Harris ratio, as ordered bits (all values > 0)
  unsigned long long* best_next;  // pass 1 sets it to "none" for the next call
  const unsigned long long* bound;  // pass 2: the bound it filters with
};

// Single-pass ordered compaction (decoupled look-back): a launch takes tiles
// of kScanTile slots in ticket order; each tile publishes its count, then its
// inclusive prefix, tagged with the launch's epoch (no reset between
// launches); the last workgroup to finish rewinds the ticket counters.
constexpr int kScanThreads = 256;
constexpr int kScanItems = 8;
constexpr int kScanTile = kScanThreads * kScanItems;
struct ScanState {
  unsigned long long* status;  // per tile: epoch << 32 | flag << 30 | count
  unsigned int* ticket;        // [0] tile ticket, [1] finished workgroups
  unsigned int epoch;          // distinct per launch, never 0
  int* fail;                   // host-visible: set if a look-back wait ran out
};

// The fused dual ratio filter + compaction writes here (mapped host memory).
struct DualSelectOut {
  int32_t* slots;      // device: kept list slots, in list order
  int* num_slots;      // device
  int32_t* cand_col;   // host-visible
  double* cand_coeff;  // host-visible
  double* cand_rc;     // host-visible
  int* counts;         // host-visible: [0] kept, [1] list length
  int host_cap;        // candidates at positions >= host_cap skip the host copy
};

// Tightening by selection (dual_tighten below): histogram passes over the
// sort keys' top 12 bits, then the next 12 within the chosen top bin, find a
// threshold with at least min(target, k1) keys at or below it (target
// kTightenTarget, MILP_TIGHTEN_TARGET in tests); one
// workgroup sorts those (at most kTightenCap) in LDS and walks them.
constexpr int kTightenTarget = 512;
constexpr int kTightenCap = 2048;
constexpr int kTightenBins = 4096;
struct TightenState {
  unsigned int hist[2][kTightenBins];
  unsigned int ticket;
  unsigned int bin0;       // pass 0: the top-12-bit bin the target falls in
  unsigned int below0;     // keys in the bins below it
  unsigned int count;      // pass 1: keys <= threshold
  unsigned long long threshold;
};

struct RowSumArgs {
  const int64_t* t_starts;
  const int32_t* t_cols;
  const double* t_vals;
  const double* x;       // multipliers per column
  const uint64_t* skip;  // optional: skip columns whose bit is set (basic)
  double sign;           // +1 (residual) or -1 (basic-value recompute)
  int num_rows;
  double* out;
};


// Batched small-LP launches (simplex_kernels.hip small_batch_kernel): one
// request per LP in a slot of mapped host memory.
enum SmallKind { kSmallRowWise = 0, kSmallColWise = 1, kSmallListDots = 2,
                 kSmallRowWiseByColumn = 3, kMediumRowWise = 4, kMediumListDots = 5,
                 kSmallKinds = 6 };
// The list dots of mid-size LPs (kMediumListDots): y (m <= kMediumListRows,
// 128 KB) staged in LDS as the small kind does.
constexpr int kMediumListRows = 16384;
struct SmallSlot {
  unsigned long long seq;  // published to done[slot] when the request is finished
  int kind;
  int pad;
  union {
    RowWiseSmallArgs rw;
    ColWiseSmallArgs cw;
    ListDotsSmallArgs ld;
    RowWiseSmallColArgs rc;
  };
};
static_assert(sizeof(SmallSlot) % 4 == 0, "the batch kernel stages a slot as 32-bit words");
constexpr int kSmallBatchMax = 128;  // requests per launch
struct SmallBatchArgs {
  const SmallSlot* slots;       // device view of the mapped slot table
  unsigned long long* done;     // device view of the mapped done words
  int count;
  int ids[kSmallBatchMax];
};

// Dense triangular solve (tri_solve.hip): TransposeLowerSolve of a
// TriangularMatrix with its outputs listed in dependency-level order and the
// values kept in that order on the device.
constexpr int kTriThreads = 1024;
constexpr int kTriPrefetch = 2;  // outputs per thread loaded ahead of their level
// Values a single-CU run of levels keeps in LDS (its own outputs): a run's
// positions never exceed this (the schedule builder cuts runs there).
constexpr int kTriLdsVals = 16384;
struct TriSolveArgs {
  const int32_t* level_start;  // [num_levels + 1] list positions of each level
  const int32_t* rec_row;      // [num_work] row (index into x) of each listed output
  const int32_t* rec_n;        // [num_work] its number of entries
  const int4* rec_entry;       // [num_work] entry positions (n <= 4) / overflow start
  const double2* rec_value;    // [2 * num_work] entry values (n <= 4)
  const double* diag;          // [num_work] diagonal, nullptr when all are 1
  const int32_t* ovf_pos;      // entries of the outputs with n > 4
  const double* ovf_value;
  const int32_t* pos_row;      // [num_pos] row of every position (listed first)
  double* x;                   // rows, in/out
  double* y;                   // [num_pos] values in position order (scratch)
  int num_work;
  int num_pos;
  int num_levels;
  int* top;                    // rows above *top are not computed (host: last non-zero)
  uint64_t* clock;             // debug (MILP_TRI_DEBUG): wall clock after each level, or null
  // Zero-copy staging (or null: the caller copies x and *top): host_x is
  // device-visible host memory holding x[first_col, num_rows) and, in the
  // int at host_x + num_rows, the top row; the plan starts by reading them
  // and ends by writing x[first_col, top] back.
  double* host_x;
  int first_col;
  int num_rows;
  int* fail;  // sync-free variant: set (host-visible) if a wait ran out
  // 0: grouped sums (TransposeLowerSolve); 1: LowerSolve's order -- one
  // subtraction per entry in list order, entries whose value is 0 skipped.
  int sequential;
  // Level plan: 1 when level 0 (outputs without entries, only a division)
  // is computed inside the gather kernel instead of a launch of its own.
  int fuse_level0;
  // Sync-free variants: a waiting lane's sleep between polls doubles from
  // one s_sleep unit up to this many (MILP_TRI_POLL_MAX; 1 = fixed).
  int poll_max;
  // A second right-hand side solved in the same launch (blockIdx.y == 1):
  // its own rows, positions, staging, top row and failure word.
  double* x2;
  double* y2;
  double* host_x2;
  int* top2;
  int* fail2;
  // Sync-free plans run the schedule as segments of consecutive levels, one
  // launch each, in order: this launch's positions are [seg_begin, seg_end).
  // A chip-wide segment (tri_syncfree_kernel) hands values between
  // workgroups through y; a narrow one (tri_chain_kernel, unpadded levels)
  // runs on one workgroup per right-hand side with its values in LDS.
  // Earlier segments are final in y when a launch starts.
  int seg_begin;
  int seg_end;
  // Sync-free plans: positions [0, level0_end) are level 0 (no entries, a
  // division at most), computed by tri_init_kernel; 0 = not fused.
  int level0_end;
};
// The argument set of right-hand side blockIdx.y (0 or 1).
__host__ __device__ inline TriSolveArgs TriRhs(const TriSolveArgs& a, int rhs) {
  TriSolveArgs b = a;
  if (rhs == 1) {
    b.x = a.x2;
    b.y = a.y2;
    b.host_x = a.host_x2;
    b.top = a.top2;
    b.fail = a.fail2;
  }
  return b;
}
// The sync-free variant needs every workgroup resident: at most this many
// outputs (512 workgroups of 256 threads, 2 per CU).
constexpr int kTriSyncFreeMaxWork = 512 * 256;
// Values the chain kernel keeps in LDS (96 KB): a tail never holds more.
constexpr int kTriChainVals = 12288;

// Dense tail of BTRAN's forward U^T solve (dense_tail.hip): upper_.
// TransposeUpperSolve (sparse.cc:848-897) when the last columns of U hold
// most of its entries (config 2's dense kernel). Columns [t, n) are the tail,
// solved by blocks of 64 columns (advance over the chip, finish on one wave).
constexpr int kTailMaxCols = 16384;
struct DenseTailArgs {
  const int64_t* starts;  // [T + 1] entry ranges of the tail columns (relative)
  const int32_t* rows;    // entries: rows (< the column)
  const double* vals;
  const double* diag;     // [T], nullptr when all are 1
  double* x;              // [n] the vector, in and out
  double* pre;            // [T] each column's running sum
  int64_t* cur;           // [T] each column's chain cursor (relative entry index)
  const double* host_x;   // device view of the pinned staging copy (n values)
  double* host_out;       // device view of the pinned output (x[t, n))
  int n;
  int t;
  int* fail;              // host-visible: a wait ran out
};

// Rows appended to the resident [A | I] (matrix_kernels.hip). The k new rows
// are the tail of the new CSR: row j holds t_cols / t_vals at [tail_starts[j],
// tail_starts[j + 1]), its structural columns ascending and its slack entry
// last. The old CSC (n structural columns, m slacks, nnz entries) is merged
// into freshly allocated arrays of nnz + e + k entries; e = the structural
// entries of the tail.
constexpr int kAppendThreads = 256;
constexpr int kAppendTileColumns = 256;  // columns per tile of the offsets scan
constexpr int kAppendShortColumn = 32;   // longer columns move on a workgroup
struct MatrixAppendArgs {
  int n, m, k;
  int64_t nnz, e;
  const int64_t* tail_starts;  // k + 1: t_starts[m ..] of the new CSR
  const int32_t* t_cols;       // the new CSR's arrays
  const double* t_vals;
  const int64_t* old_starts;   // n + m + 1
  const int32_t* old_rows;
  const double* old_vals;
  int64_t* new_starts;         // n + m + k + 1
  int32_t* new_rows;
  double* new_vals;
  int* add;                    // n: new entries per column (zeroed by the caller)
  int* rank;                   // e + k: earlier new rows that hold the entry's column
  int tiles;                   // ceil((n + 1) / kAppendTileColumns)
  int* tile_counts;            // tiles
  int64_t* tile_offsets;       // tiles
};

// Rows deleted from the resident [A | I] (matrix_kernels.hip). delete_mask has
// m bytes, non-zero deletes the row (the mask of mi_lp_delete_rows as it is).
// The old CSC (n structural columns, m slacks) and CSR are compacted into
// freshly allocated arrays; the host knows the new shape from its own
// compacted pair: kept rows and the structural entries left.
constexpr int kDeleteThreads = 256;
constexpr int kDeleteTile = 256;         // rows or columns per tile of the scans
constexpr int kDeleteShort = 32;         // longer columns / rows move on a workgroup
struct MatrixDeleteArgs {
  int n, m, kept;
  int64_t new_structural;      // entries of the new structural columns
  const uint8_t* delete_mask;  // m
  const int64_t* old_starts;   // n + m + 1
  const int32_t* old_rows;
  const double* old_vals;
  const int64_t* old_t_starts; // m + 1
  const int32_t* old_t_cols;
  const double* old_t_vals;
  int64_t* new_starts;         // n + kept + 1
  int32_t* new_rows;
  double* new_vals;
  int64_t* new_t_starts;       // kept + 1
  int32_t* new_t_cols;
  double* new_t_vals;
  int* new_row;                // m: the kept rows below r
  int* count;                  // n: kept entries per structural column
  int row_tiles, col_tiles;    // ceil(m / kDeleteTile), ceil(n / kDeleteTile)
  int* row_tile_rows;          // row_tiles: kept rows of the tile, then those before it
  int64_t* row_tile_entries;   // row_tiles: their CSR entries, likewise
  int64_t* col_tile_entries;   // col_tiles: kept entries of the tile, then before it
};
}  // namespace milp_kernels

namespace milp_launch {
// The merge of MatrixAppendArgs in stream order: rank and count, tile counts,
// tile offsets, starts, then the moves (short columns one per thread; with
// long_columns also one workgroup per column longer than kAppendShortColumn)
// and the scatter of the new entries and slacks.
hipError_t matrix_append_rows(const milp_kernels::MatrixAppendArgs& args, bool long_columns,
                              hipStream_t s);
// The compaction of MatrixDeleteArgs in stream order: the row map and the new
// CSR starts (count per tile, one workgroup over the tile counts, starts per
// tile), the CSR moves, the kept entries per column, the CSC starts by the
// same three passes, the CSC moves and the slack columns. long_rows /
// long_columns: some kept row / old structural column is longer than
// kDeleteShort and the workgroup kernels run as well.
hipError_t matrix_delete_rows(const milp_kernels::MatrixDeleteArgs& args, bool long_columns,
                              bool long_rows, hipStream_t s);
hipError_t column_dot(int mode, bool wave_per_col, const milp_kernels::DotArgs& args,
                      hipStream_t s);
// unroll: 16-byte loads in flight per lane (8, 16 or 32).
hipError_t dense_dot(int mode, int unroll, const milp_kernels::DenseArgs& args, hipStream_t s);
// The same dots for a panel of `width` (1, 4 or 16) vectors in one pass over
// the columns (panel_kernels.hip). long_columns: one wave per column (the
// wave_per_col shape of column_dot), else 4 * width lanes per column.
hipError_t column_dot_panel(int width, bool long_columns, const milp_kernels::PanelDotArgs& args,
                            hipStream_t s);
hipError_t dense_dot_panel(int width, const milp_kernels::PanelDenseArgs& args, hipStream_t s);
// out[v * ld + col] = in[col * width + v] for v < kp, col < ncols.
hipError_t panel_deinterleave(int width, const double* in, int ncols, int kp, double* out,
                              int64_t ld, hipStream_t s);
// panel_count, panel_offsets and panel_write for one panel, in that order.
hipError_t panel_sparse(int width, const milp_kernels::PanelSparseArgs& args, hipStream_t s);
// penalties_tile, then penalties_fold (kp workgroups), on one stream.
hipError_t panel_penalties(int width, const milp_kernels::PenaltyArgs& args, hipStream_t s);
// gomory_transform_tile over the first pass' result; then, after the caller's
// second dot pass, gomory_combine_tile and gomory_fold (kp workgroups).
hipError_t panel_gomory_transform(int width, const milp_kernels::GomoryArgs& args, hipStream_t s);
hipError_t panel_gomory_combine(int width, const milp_kernels::GomoryArgs& args, hipStream_t s);
// Row sums for a panel of `width` (1, 4 or 16) points in one pass over the
// rows of [A | I] (panel_kernels.hip row_sums_panel_kernel).
hipError_t row_sums_panel(int width, const milp_kernels::RowPanelArgs& args, hipStream_t s);
// out[col * width + v] = in[v * ld + col] for v < kp, 0.0 for kp <= v < width.
hipError_t panel_interleave(int width, const double* in, int64_t ld, int ncols, int kp,
                            double* out, hipStream_t s);
// out[col * width + v] = base[col] for v < kp, 0.0 for kp <= v < width.
hipError_t panel_fill(int width, const double* base, int ncols, int kp, double* out,
                      hipStream_t s);
// num_overrides = starts[kp] - starts[0] (known to the host).
hipError_t panel_override(int width, const milp_kernels::RowPanelOverrideArgs& args,
                          int64_t num_overrides, hipStream_t s);
// After row_sums_panel on the same stream: violations_count, then (rows !=
// nullptr) panel_offsets, (summaries != nullptr) violations_fold, and (rows
// != nullptr) violations_write, all under `rule` (PanelRowRule).
hipError_t row_violations_panel(int width, int rule, const milp_kernels::RowViolationArgs& args,
                                hipStream_t s);
// Activity ranges for a panel of `width` (1, 4 or 16) bound sets in one pass
// over the rows of [A | I] (panel_kernels.hip activity_ranges_panel_kernel).
hipError_t activity_ranges_panel(int width, const milp_kernels::ActivityRangeArgs& args,
                                 hipStream_t s);
// After activity_ranges_panel (dense mode) on the same stream: the implied
// bounds of the structural columns for the same panel. long_columns: one
// workgroup per column, else 256 / width columns per workgroup
// (panel_kernels.hip implied_bounds_panel_kernel).
hipError_t implied_bounds_panel(int width, bool long_columns,
                                const milp_kernels::ImpliedBoundsArgs& args, hipStream_t s);
// After row_violations_panel under kRowRuleKeptKey with lists.
hipError_t implied_gather(int width, const milp_kernels::ImpliedGatherArgs& args, hipStream_t s);
// After implied_bounds_panel on the same stream: the round applied to the own
// bounds in place, and its keys (panel_kernels.hip propagate_apply_panel_kernel).
hipError_t propagate_apply(int width, const milp_kernels::PropagateApplyArgs& args,
                           hipStream_t s);
// The keys of the final bounds against the base (propagate_changed_keys_kernel).
hipError_t propagate_changed_keys(int width, const milp_kernels::PropagateChangedArgs& args,
                                  hipStream_t s);
hipError_t dense_pack(const int64_t* starts, const double* vals, const int32_t* dense_cols,
                      int nd, int m, double* body, double* tail, hipStream_t s);
hipError_t gather(const int32_t* list, int n, const double* src, double* dst, hipStream_t s);
// Flags -> ascending list + coefficient gather + count, one workgroup, for
// n <= kSmallCompactMax.
constexpr int kSmallCompactMax = 1 << 14;  // one workgroup writes the list to host memory
hipError_t compact_small(const uint8_t* flags, int n, const double* coeff,
                         const milp_kernels::ListOut& out, hipStream_t s);
// Any n: flags -> ascending list + coefficients + count in one launch
// (ordered single-pass compaction).
hipError_t compact_flags(const uint8_t* flags, int n, const double* coeff,
                         const milp_kernels::ListOut& out, const milp_kernels::ScanState& st,
                         hipStream_t s);
// Tiles a compaction launch over n slots uses (ScanState::status length).
inline int scan_tiles(int n) {
  return n <= 0 ? 1 : (n + milp_kernels::kScanTile - 1) / milp_kernels::kScanTile;
}
hipError_t row_wise_update(const milp_kernels::RowWiseArgs& args, hipStream_t s);
// entries: the filtered rows' total length (<= kListEntriesMax).
hipError_t row_wise_list(const milp_kernels::RowWiseListArgs& args, int entries, hipStream_t s);
// flags[list[i]] = 1 for i < *count (flags cleared by the caller; max_count
// sizes the grid).
hipError_t flags_from_list(const int32_t* list, const int* count, int max_count, uint8_t* flags,
                           hipStream_t s);
// threads: 1024, or 256 (used when the filtered rows fit one per thread).
hipError_t row_wise_update_small(const milp_kernels::RowWiseSmallArgs& args, int threads,
                                 hipStream_t s);
hipError_t row_wise_update_medium(const milp_kernels::RowWiseSmallArgs& args, hipStream_t s);
hipError_t small_batch(int kind, const milp_kernels::SmallBatchArgs& args, hipStream_t s);
hipError_t list_dots_small(const milp_kernels::ListDotsSmallArgs& args, hipStream_t s);
hipError_t list_dots_medium(const milp_kernels::ListDotsSmallArgs& args, hipStream_t s);
hipError_t row_wise_update_small_by_column(const milp_kernels::RowWiseSmallColArgs& args,
                                           hipStream_t s);
hipError_t column_wise_update_small(const milp_kernels::ColWiseSmallArgs& args, hipStream_t s);
// Marks the filtered rows (row_tag[r] = tag, row_pos[r] = list position).
hipError_t tag_rows(const int32_t* filtered_rows, int num_filtered, uint32_t tag,
                    uint32_t* row_tag, int32_t* row_pos, hipStream_t s);
hipError_t row_wise_update_by_column(const milp_kernels::RowWiseColArgs& args, hipStream_t s);
hipError_t row_wise_update_full_rows(const milp_kernels::RowWiseFullArgs& args, hipStream_t s);
hipError_t row_sums(const milp_kernels::RowSumArgs& args, hipStream_t s);
// Dual device mode.
hipError_t dual_ratio_bound(const milp_kernels::DualRatioArgs& args, hipStream_t s);
// Pass 2 fused with its compaction and the candidate gather: the eligible
// slots with ratio <= *args.bound (1 + 1e-9), in list order, one launch.
hipError_t dual_ratio_select(const milp_kernels::DualRatioArgs& args,
                             const milp_kernels::DualSelectOut& out,
                             const milp_kernels::ScanState& st, hipStream_t s);
// Both passes in one launch of one workgroup, for lists of at most
// kDualOneWgMax slots (args.max_count): the block minimum B goes to
// *args.best (where the tightening round reads it), the selection as above.
constexpr int kDualOneWgMax = 8192;
hipError_t dual_ratio_one_wg(const milp_kernels::DualRatioArgs& args,
                             const milp_kernels::DualSelectOut& out, hipStream_t s);
// Tighter bound: sort keys (ratio, order-preserving bits) of the pass-2 slots.
hipError_t dual_ratio_keys(const milp_kernels::DualRatioArgs& args, const int32_t* slots,
                           int num_slots, unsigned long long* keys, hipStream_t s);
// Walks the ratio-sorted breakpoints the way the second Glop loop pops them
// (flipping boxed ones while the variation stays positive) up to the first
// accepted breakpoint; *bound2 = min(B, its Harris ratio) (or B = *args.best
// on a ratio tie, where the pop order also depends on magnitudes).
hipError_t dual_flip_walk(const milp_kernels::DualRatioArgs& args, const int32_t* sorted_slots,
                          int num_slots, unsigned long long* bound2, hipStream_t s);
// The same bound from the smallest keys only (keys, two histogram passes,
// one sort-and-walk workgroup): bound2[0] is the full walk's result, or B
// when the walk leaves the gathered prefix; bound2[1] the walk length
// (statistics). Uses `keys` (num_slots entries) and `st` as scratch.
hipError_t dual_tighten(const milp_kernels::DualRatioArgs& args, const int32_t* slots,
                        int num_slots, unsigned long long* keys, milp_kernels::TightenState* st,
                        unsigned long long* bound2, int target_keys, hipStream_t s);
// rc[list[i]] += mult * list_coeff[i] (reduced_costs.cc:466-470), then
// rc[leaving] = leaving_value, rc[entering] = 0.
hipError_t update_reduced_costs(const int32_t* list, const double* list_coeff, const int* count,
                                int max_count, double mult, int leaving_col,
                                double leaving_value, int entering_col, double* rc,
                                hipStream_t s);
hipError_t set_double(double* dst, double value, hipStream_t s);
// colbits[cols[i]] = bits[i].
hipError_t set_colbits(const int32_t* cols, const uint8_t* bits, int n, uint8_t* colbits,
                       hipStream_t s);
// MakeBoxedVariableDualFeasible (revised_simplex.cc:2391-2437) decisions:
// flag[i] = new status (AT_LOWER/AT_UPPER) if cols[i] flips, else 0xff.
// cols == nullptr: every column whose bit 2 (non-basic boxed) is set.
hipError_t set_mask_words(const int32_t* idx, const uint64_t* words, int n, uint64_t* mask,
                          hipStream_t s);
hipError_t boxed_flips(const int32_t* cols, int n, const double* rc, const uint8_t* colbits,
                       double threshold, uint8_t* flag, hipStream_t s);
// segments: num_segments pairs; (lb, le) with lb >= 0 = levels [lb, le) on
// one CU; (-level - 1, blocks) = one wide level over `blocks` workgroups.
hipError_t tri_transpose_lower(const milp_kernels::TriSolveArgs& args, const int* segments,
                               int num_segments, hipStream_t s);
// The same solve driven by per-output readiness instead of levels
// (rec_row/x updated in place, no scatter): one launch per segment, segs =
// num_segs triples (first position, end position, 1 = narrow segment on one
// workgroup / 0 = chip-wide).
hipError_t tri_transpose_lower_syncfree(const milp_kernels::TriSolveArgs& args,
                                        const int* segs, int num_segs, hipStream_t s,
                                        int num_rhs = 1);
// The same, persistent: `groups` workgroups of kTriThreads threads walk the
// outputs in level order (thread t: t, t + T, ...); xcd_stride 8 keeps them
// on one XCD under round-robin dealing (speed only, any placement is correct).
hipError_t tri_transpose_lower_persistent(const milp_kernels::TriSolveArgs& args, int groups,
                                          int xcd_stride, hipStream_t s);
hipError_t column_squared_norms(const int64_t* starts, const double* vals,
                                const uint64_t* relevant, int ncols, double* out,
                                hipStream_t s);
// Dense-tail TransposeUpperSolve: copy-in of x from host_x, the blocks of
// 64 tail columns (advance + finish launches), copy-out of x[t, n) to host_out.
hipError_t dense_tail_upper_solve(const milp_kernels::DenseTailArgs& args, hipStream_t s);

}  // namespace milp_launch

#endif  // MILP_KERNEL_ARGS_H_
