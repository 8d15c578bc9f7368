/* TEST SUPPORT ONLY: one DeviceLp operation at a time, with inputs the caller
 * chooses. Not part of the solver API of include/mi_lp.h.
 *
 * A mi_devop handle owns the matrix pair [A | I] (CSC and its transpose) and a
 * DeviceLp of its own; there is no RevisedSimplex behind it. create() reads
 * the MILP_* environment switches (DeviceLp::Init), so a test sets the
 * environment first and creates the handle afterwards.
 *
 * The library exports read-only tables, mi_devop_table and (for the matrix
 * entries at the end of this file) mi_devop_matrix_table, instead of one
 * function per call: the exported functions of libmi_lp.so stay exactly those
 * of mi_lp.h. Every call returns 0, or non-zero with a message in
 * last_error(h) (a failed create: last_error(NULL), per thread). No C++
 * exception crosses this boundary.
 *
 * Preconditions are DeviceLp's own and are not checked here: filtered rows
 * ascend and are in range, column indices are in range, vectors have m (rho,
 * w, v, y) or N = n + m (rc, colbits, bound_diff, c, x, out) elements. The
 * fused pricing (w given) and list_dots_over_update_row need the list's count:
 * fetch_update_row comes first. The dual_* calls need dual_begin first;
 * dual_take_priced_reduced_costs needs a pricing call before it, and
 * dual_set_reduced_cost a column in [0, N). */
#ifndef MI_LP_DEVOP_H_
#define MI_LP_DEVOP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi_devop mi_devop;

/* DeviceLp::LastPaths: which kernels the last operations went through. */
enum {
  MI_DEVOP_ROW_NONE = 0,
  MI_DEVOP_ROW_SMALL_SERIAL = 1,
  MI_DEVOP_ROW_SMALL_SERIAL_256 = 2,
  MI_DEVOP_ROW_SMALL_BY_COLUMN = 3,
  MI_DEVOP_ROW_MEDIUM_DIRECT = 4,
  MI_DEVOP_ROW_MEDIUM_BATCHED = 5,
  MI_DEVOP_ROW_LIST = 6,
  MI_DEVOP_ROW_FULL_ROWS = 7,
  MI_DEVOP_ROW_CHUNK = 8,
  MI_DEVOP_ROW_BY_COLUMN = 9,
  MI_DEVOP_ROW_COLUMN_WISE_SMALL = 10,
  MI_DEVOP_ROW_COLUMN_WISE_GENERAL = 11
};
enum { MI_DEVOP_COMPACT_NONE = 0, MI_DEVOP_COMPACT_SMALL = 1, MI_DEVOP_COMPACT_CHIP_WIDE = 2 };
enum { MI_DEVOP_RATIO_NONE = 0, MI_DEVOP_RATIO_ONE_WORKGROUP = 1, MI_DEVOP_RATIO_TWO_KERNELS = 2 };

typedef struct mi_devop_paths {
  int32_t update_row;      /* MI_DEVOP_ROW_* of the last update row */
  int32_t compact;         /* MI_DEVOP_COMPACT_* of that update row */
  int32_t ratio;           /* MI_DEVOP_RATIO_* of the last dual ratio test */
  int32_t ratio_tightened; /* it ran the tightening round */
  int32_t list_mapped;     /* the last list also went to the mapped host mirrors */
} mi_devop_paths;

/* DeviceLp::LastPanel: which kernels the last column_dots_panel went through. */
enum { MI_DEVOP_PANEL_NONE = 0, MI_DEVOP_PANEL_SHORT_COLUMNS = 1, MI_DEVOP_PANEL_LONG_COLUMNS = 2 };
typedef struct mi_devop_panel {
  int32_t sparse; /* MI_DEVOP_PANEL_* of the CSC kernel */
  int32_t dense;  /* the dense-block kernel ran */
  int32_t panels; /* panels of up to 16 vectors */
  int32_t width;  /* padded width of the last panel: 1, 4 or 16 */
} mi_devop_panel;

/* DeviceLp::LastPanelSparse: the last column_dots_panel_sparse. */
typedef struct mi_devop_panel_sparse {
  int32_t sparse; /* as mi_devop_panel */
  int32_t dense;
  int32_t panels;
  int32_t width;
  int64_t kept;       /* entries of all rows */
  int64_t bytes_down; /* device-to-host bytes of the call */
} mi_devop_panel_sparse;
/* The two constants of the sparse-row kernels (kernels/kernel_args.h). */
typedef struct mi_devop_panel_sparse_geometry {
  int32_t tile_columns;       /* columns of one workgroup's tile */
  int32_t offsets_step_tiles; /* tiles per block scan of the offsets kernel */
} mi_devop_panel_sparse_geometry;
/* column_dots_panel_sparse: the result needs more than `capacity` entries. */
enum { MI_DEVOP_CAPACITY = 2 };

/* mi_lp_branch_penalty of include/mi_lp.h, restated so that this header
 * stands alone. */
typedef struct mi_devop_branch_penalty {
  double down;
  double up;
  int32_t down_col; /* -1 when down_count == 0 */
  int32_t up_col;
  int32_t down_count;
  int32_t up_count;
} mi_devop_branch_penalty;
/* DeviceLp::LastPenalties: the last column_penalties_panel. */
typedef struct mi_devop_penalties {
  int32_t sparse; /* as mi_devop_panel */
  int32_t dense;
  int32_t panels;
  int32_t width;
  int32_t tiles; /* tiles of tile_columns columns per panel (summed over column shards) */
  int32_t reserved;
  int64_t bytes_down; /* device-to-host bytes of the call */
} mi_devop_penalties;

/* mi_lp_cut_summary of include/mi_lp.h, restated so that this header stands
 * alone. */
typedef struct mi_devop_cut_summary {
  double max_abs;
  double min_abs;
  int32_t count;
  int32_t bad_count;
  int32_t max_col; /* -1 when count == 0 */
  int32_t min_col;
} mi_devop_cut_summary;
/* DeviceLp::LastCuts: the last column_cuts_panel. */
typedef struct mi_devop_cuts {
  int32_t sparse; /* as mi_devop_panel */
  int32_t dense;
  int32_t panels;
  int32_t width;
  int32_t tiles;            /* tiles of tile_columns columns over all N columns */
  int32_t structural_tiles; /* over the n structural columns */
  int32_t lists;            /* lists were built */
  int32_t reserved;
  int64_t kept;       /* entries of all cuts */
  int64_t bytes_down; /* device-to-host bytes of the call */
} mi_devop_cuts;

/* TriKind of engine/device_solver.h: the host loop a device solve replaces. */
enum {
  MI_DEVOP_TRI_UPPER_T = 0,    /* TransposeLowerSolve (entries from the column's end) */
  MI_DEVOP_TRI_LOWER = 1,      /* LowerSolveStartingAt (column scatter) */
  MI_DEVOP_TRI_UPPER_T_UP = 2, /* TransposeUpperSolve (entries from the column's start) */
  MI_DEVOP_TRI_LOWER_T = 3,    /* TransposeLowerSolve */
  MI_DEVOP_TRI_UNIT_ROW = 4,   /* LowerSolveStartingAt */
  MI_DEVOP_TRI_UPPER = 5       /* UpperSolve (backward column scatter) */
};
/* DeviceLp::TriPlan. */
enum {
  MI_DEVOP_TRI_PLAN_NONE = 0, /* refused: the host loop runs */
  MI_DEVOP_TRI_PLAN_TRIVIAL = 1, /* nothing to compute, no launch */
  MI_DEVOP_TRI_PLAN_SYNC_FREE = 2,
  MI_DEVOP_TRI_PLAN_PERSISTENT = 3,
  MI_DEVOP_TRI_PLAN_LEVELS = 4,
  MI_DEVOP_TRI_PLAN_DENSE_TAIL = 5
};
/* DeviceLp::LastTri: the last tri_solve, tri_solve_pair or tri_async_begin. */
typedef struct mi_devop_tri {
  int32_t plan; /* MI_DEVOP_TRI_PLAN_* */
  int32_t kind; /* MI_DEVOP_TRI_* of the schedule */
  int32_t rows;
  int32_t first_col;    /* first output of the schedule */
  int32_t top;          /* last row the solve computes */
  int32_t work;         /* listed outputs and padding */
  int32_t pos;          /* positions: work + the rows only read */
  int32_t levels;
  int32_t chain_levels; /* levels in single-workgroup segments */
  int32_t level0_end;   /* positions of a chip-wide level 0 */
  int32_t wide_runs;    /* sync-free plan: chip-wide launches */
  int32_t chain_runs;   /* sync-free plan: single-workgroup launches */
  int32_t chip_launches; /* level plan: levels launched alone over the chip */
  int32_t cu_runs;      /* level plan: single-CU runs of narrow levels */
  int32_t fused0;       /* level 0 computed by the gather or init kernel */
  int32_t vectors;      /* right-hand sides of the launch (2: a pair) */
  int32_t max_wide_run; /* positions of the largest chip-wide segment */
  int32_t max_entries;
  int32_t rows_over[3]; /* outputs of more than 4, 16, 64 entries */
  int32_t t;            /* dense tail: its first column */
  int32_t tail_cols;    /* dense tail: T = rows - t */
  int32_t blocks;       /* dense tail: ceil(T / 64) */
  int64_t entries;      /* dense tail: entries of its columns */
} mi_devop_tri;

/* DeviceLp::LastAppend: the last append_rows. */
enum { MI_DEVOP_MOVE_COLUMN_PER_THREAD = 1, MI_DEVOP_MOVE_COLUMN_PER_WORKGROUP = 2 };
typedef struct mi_devop_append {
  int32_t path;        /* 1 merged on the device, 2 full upload */
  int32_t rows;        /* k */
  int64_t entries;     /* structural entries of the new rows */
  int64_t bytes_up;    /* host -> device for the matrix */
  int32_t move_shapes; /* MI_DEVOP_MOVE_* bits of the move kernels that ran */
  int32_t reserved;
  double device_ms;    /* copies and merge kernels, by events */
} mi_devop_append;

/* DeviceLp::LastColumnDots: the last launch of the column-dot kernels. */
typedef struct mi_devop_column_dots {
  int32_t mode;         /* DotMode of simplex_kernels.hip: 1 pricing, 5 pricing with dots */
  int32_t wave_per_col; /* the long-column CSC kernel (else four lanes per column) */
  int32_t dense;        /* the dense-block kernel ran */
  int32_t dense_unroll; /* its variant: 8, 16 or 32 (0 without a dense block) */
} mi_devop_column_dots;
/* DeviceLp::LastFlips: the last dual_boxed_flips. */
typedef struct mi_devop_flips {
  int32_t early_taken; /* it returned the flags of dual_boxed_flips_early's launch */
} mi_devop_flips;

/* DeviceLp::LastRowPanel: the last row_sums_panel / row_sums_panel_from. */
enum { MI_DEVOP_ROW_PANEL_NONE = 0, MI_DEVOP_ROW_PANEL_DIRECT = 1 };
typedef struct mi_devop_row_panel {
  int32_t panels;             /* panels of up to 16 points */
  int32_t width;              /* padded width of the last panel: 1, 4 or 16 */
  int32_t kernel;             /* MI_DEVOP_ROW_PANEL_* of the last panel */
  int32_t reserved;
  int64_t overrides_up_bytes; /* host-to-device bytes of a row_sums_panel_from call */
} mi_devop_row_panel;
/* row_sums_panel_kernel's shape (kernels/kernel_args.h). */
typedef struct mi_devop_row_panel_geometry {
  int32_t rows_per_workgroup[3]; /* at widths 1, 4 and 16 */
  int32_t chunk;                 /* staging chunk length; 0: the kernel does not stage */
} mi_devop_row_panel_geometry;

/* mi_lp_point_violations of include/mi_lp.h, restated so that this header
 * stands alone. */
typedef struct mi_devop_point_violations {
  int64_t count;
  double worst;
  int32_t worst_row; /* -1 when count == 0 */
  int32_t reserved;
} mi_devop_point_violations;
/* DeviceLp::LastRowViolations: the last row_violations_panel(_from). */
typedef struct mi_devop_row_violations {
  int32_t panels;             /* panels of up to 16 points */
  int32_t width;              /* padded width of the last panel: 1, 4 or 16 */
  int32_t lists;              /* lists were built (row_starts given) */
  int32_t reserved;
  int64_t kept;               /* entries of all points */
  int64_t bytes_down;         /* device-to-host bytes of the call */
  int64_t overrides_up_bytes; /* host-to-device bytes of a row_violations_panel_from call */
} mi_devop_row_violations;
/* DeviceLp::LastBoundImplied: the last bound_implied_panel(_from) or
 * bound_tightened_panel(_from). */
typedef struct mi_devop_bound_implied {
  int32_t panels;     /* panels of up to 16 bound sets */
  int32_t width;      /* padded width of the last panel: 1, 4 or 16 */
  int32_t columns;    /* MI_DEVOP_PANEL_SHORT_COLUMNS or MI_DEVOP_PANEL_LONG_COLUMNS */
  int32_t lists;      /* lists were built (col_starts given) */
  int64_t kept;       /* entries of all sets */
  int64_t bytes_up;   /* host-to-device bytes of the call: the sets and 16 m of row bounds */
  int64_t bytes_down; /* device-to-host bytes of the call */
} mi_devop_bound_implied;
/* mi_lp_propagation of include/mi_lp.h, restated so that this header stands
 * alone. */
typedef struct mi_devop_propagation {
  int32_t status; /* 0 round limit, 1 fixpoint, 2 infeasible */
  int32_t rounds;
  int64_t moves;
  double worst;
  int32_t worst_col; /* -1 unless infeasible */
  int32_t kept;
} mi_devop_propagation;
/* Parameters of the propagate entries. is_integer: n bytes, or NULL. */
typedef struct mi_devop_propagate_params {
  const uint8_t* is_integer;
  double tolerance;             /* finite, >= 0 (checked by the entries) */
  double integrality_tolerance; /* in [0, 0.5) */
  int32_t max_rounds;           /* >= 1 */
  int32_t reserved;
} mi_devop_propagate_params;
/* DeviceLp::LastBoundPropagate: the last bound_propagate_panel(_from) or
 * bound_propagated_columns_from. */
typedef struct mi_devop_bound_propagate {
  int32_t panels;     /* panels of up to 16 bound sets */
  int32_t width;      /* padded width of the last panel: 1, 4 or 16 */
  int32_t columns;    /* implied-bound kernel shape of the last panel */
  int32_t lists;      /* lists were built (col_starts given) */
  int64_t rounds;     /* rounds launched, summed over the panels */
  int64_t kept;       /* entries of all lists */
  int64_t bytes_up;   /* the sets, 16 m of row bounds and n of is_integer */
  int64_t bytes_down; /* 24 per set and round (twice in a round 1 that finds a crossing),
                         then the results */
} mi_devop_bound_propagate;

typedef struct mi_devop_api {
  /* A (m x n) in CSC; the m slack columns are appended. NULL on failure. */
  mi_devop* (*create)(int device, int m, int n, const int64_t* col_starts,
                      const int32_t* row_idx, const double* vals);
  void (*destroy)(mi_devop* h);
  const char* (*last_error)(const mi_devop* h);
  /* which: DeviceLp::Mask (0 relevant, 1 basic, 2 not basic). */
  int (*set_mask)(mi_devop* h, int which, const uint64_t* words, int num_words);
  int (*set_list_mirror)(mi_devop* h, int on);
  int (*set_small_batch)(mi_devop* h, int on);
  int (*update_row_row_wise)(mi_devop* h, const int32_t* rows, int k, const double* rho,
                             int algorithm, double drop);
  /* relevant_entries is computed from the last relevant mask. w may be NULL. */
  int (*update_row_column_wise)(mi_devop* h, const double* rho, double drop, const double* w);
  /* positions / values hold N elements. */
  int (*fetch_update_row)(mi_devop* h, int32_t* positions, double* values, int* count);
  int (*read_coefficient)(mi_devop* h, int col, double* out);
  int (*download_coefficients)(mi_devop* h, double* out);
  int (*list_dots_over_update_row)(mi_devop* h, const double* v, double* out, int* count);
  int (*list_dots)(mi_devop* h, const int32_t* cols, int n, const double* v, double* out);
  int (*dual_begin)(mi_devop* h, const double* rc, const uint8_t* colbits,
                    const double* bound_diff);
  int (*dual_set_col_bits)(mi_devop* h, const int32_t* cols, const uint8_t* bits, int n);
  /* col / coeff / rc hold N elements. */
  int (*dual_ratio_candidates)(mi_devop* h, double sign, double threshold,
                               double harris_tolerance, double minimum_delta,
                               double variation_magnitude, int32_t* col, double* coeff,
                               double* rc, int* count, int* list_count);
  int (*dual_update_reduced_costs)(mi_devop* h, double mult, int leaving_col,
                                   double leaving_value, int entering_col);
  int (*dual_download_reduced_costs)(mi_devop* h, double* rc);
  int (*last_paths)(mi_devop* h, mi_devop_paths* out);
  /* Appended after last_paths: the entries above keep their places.
   * y: k x m, out: k x N, both vector-major (DeviceLp::ColumnDotsPanel). */
  int (*column_dots_panel)(mi_devop* h, const double* y, int k, double* out);
  int (*last_panel)(mi_devop* h, mi_devop_panel* out);
  /* Measurement only: device-event milliseconds of the panel kernels and of
   * the list_dots kernels since the previous call (the first call turns the
   * event timing on and returns zeros). */
  int (*take_kernel_ms)(mi_devop* h, double* panel_ms, double* list_dots_ms);
  /* Appended after take_kernel_ms. DeviceLp::ColumnDotsPanelSparse in one
   * call: row j of the k rows keeps, columns ascending, the columns whose bit
   * is set in keep_mask_words (ceil(N / 64) words, NULL: all) with
   * fabs(dot) > drop_tolerance. row_starts: k + 1; cols / vals: `capacity`
   * entries. A result of more than `capacity` entries returns
   * MI_DEVOP_CAPACITY (last_error says how many) with row_starts, cols and
   * vals unwritten; it is no device error. */
  int (*column_dots_panel_sparse)(mi_devop* h, const double* y, int k, double drop_tolerance,
                                  const uint64_t* keep_mask_words, int64_t* row_starts,
                                  int32_t* cols, double* vals, int64_t capacity);
  int (*last_panel_sparse)(mi_devop* h, mi_devop_panel_sparse* out);
  int (*panel_sparse_geometry)(mi_devop_panel_sparse_geometry* out);
  /* Appended after panel_sparse_geometry. DeviceLp::Pricing: rc_out[N] =
   * c - A^T y. With w != NULL the same pass computes a_j . w over the last
   * update row's list: list_dots_out (N elements) receives *list_count dots
   * in list order. w == NULL: *list_count = 0, list_dots_out is not touched. */
  int (*pricing)(mi_devop* h, const double* c, const double* y, const double* w, double* rc_out,
                 double* list_dots_out, int* list_count);
  /* out[N]; only the positions of the last relevant mask are defined. */
  int (*column_squared_norms)(mi_devop* h, double* out);
  /* out[m]; skip_basic: the columns of the kBasic mask (set_mask which 1). */
  int (*row_sums)(mi_devop* h, const double* x, int skip_basic, double sign, double* out);
  /* cols == NULL: every column, flags_out holds N bytes; else n bytes. */
  int (*dual_boxed_flips)(mi_devop* h, const int32_t* cols, int n, double threshold,
                          uint8_t* flags_out);
  int (*dual_boxed_flips_early)(mi_devop* h, const int32_t* cols, int n, double threshold);
  int (*dual_take_priced_reduced_costs)(mi_devop* h);
  int (*dual_set_reduced_cost)(mi_devop* h, int col, double value);
  int (*last_column_dots)(mi_devop* h, mi_devop_column_dots* out);
  int (*last_flips)(mi_devop* h, mi_devop_flips* out);
  /* Appended after last_flips. x: k x N, out: k x m, both vector-major
   * (DeviceLp::RowSumsPanel). */
  int (*row_sums_panel)(mi_devop* h, const double* x, int k, double* out);
  /* base: N; starts: k + 1; cols / vals: starts[k] entries, NULL when that is
   * 0 (DeviceLp::RowSumsPanelFrom). Checked here, since a bad column would be
   * a store out of bounds: starts[0] == 0, starts non-decreasing, columns in
   * [0, N), no column twice within a point. */
  int (*row_sums_panel_from)(mi_devop* h, const double* base, int k, const int64_t* starts,
                             const int32_t* cols, const double* vals, double* out);
  int (*last_row_panel)(mi_devop* h, mi_devop_row_panel* out);
  int (*row_panel_geometry)(mi_devop_row_panel_geometry* out);
  /* Appended after row_panel_geometry. DeviceLp::RowViolationsPanel in one
   * call (the rule: include/mi_lp.h mi_lp_column_combinations_violations). x:
   * k x N; row_lb / row_ub: m each, not NULL, no NaN, row_lb < +inf and
   * row_ub > -inf; tolerance finite and >= 0 (checked here). row_starts:
   * k + 1; rows / activities: `capacity` entries; summaries: k, or NULL.
   * row_starts == NULL selects summaries only: rows and activities are not
   * touched. A result of more than `capacity` entries returns
   * MI_DEVOP_CAPACITY (last_error says how many) with row_starts, rows,
   * activities and summaries unwritten; it is no device error. */
  int (*row_violations_panel)(mi_devop* h, const double* x, int k, const double* row_lb,
                              const double* row_ub, double tolerance, int64_t* row_starts,
                              int32_t* rows, double* activities, int64_t capacity,
                              mi_devop_point_violations* summaries);
  /* base, starts, cols, vals and their checks as row_sums_panel_from. */
  int (*row_violations_panel_from)(mi_devop* h, const double* base, int k, const int64_t* starts,
                                   const int32_t* cols, const double* vals, const double* row_lb,
                                   const double* row_ub, double tolerance, int64_t* row_starts,
                                   int32_t* rows, double* activities, int64_t capacity,
                                   mi_devop_point_violations* summaries);
  int (*last_row_violations)(mi_devop* h, mi_devop_row_violations* out);
  /* Appended after last_row_violations. DeviceLp::BoundRangesPanel (the rule:
   * include/mi_lp.h mi_lp_bound_activity_ranges). lbs / ubs: k x n over the
   * structural columns; min_activity / max_activity: k x m; inf_counts:
   * k x m x 2, or NULL. */
  int (*bound_ranges_panel)(mi_devop* h, const double* lbs, const double* ubs, int k,
                            double* min_activity, double* max_activity, int32_t* inf_counts);
  /* base_lb / base_ub: n; starts: k + 1; cols / new_lbs / new_ubs: starts[k]
   * entries, NULL when that is 0. Checked here as row_sums_panel_from does,
   * with the columns in [0, n). */
  int (*bound_ranges_panel_from)(mi_devop* h, const double* base_lb, const double* base_ub, int k,
                                 const int64_t* starts, const int32_t* cols,
                                 const double* new_lbs, const double* new_ubs,
                                 double* min_activity, double* max_activity,
                                 int32_t* inf_counts);
  /* DeviceLp::BoundInfeasiblePanel in one call. row_lb / row_ub: m each, not
   * NULL, no NaN (+-inf allowed on either side); tolerance finite and >= 0
   * (checked here). row_starts, rows, amounts, capacity and summaries as
   * row_violations_panel, MI_DEVOP_CAPACITY included. */
  int (*bound_infeasible_panel)(mi_devop* h, const double* lbs, const double* ubs, int k,
                                const double* row_lb, const double* row_ub, double tolerance,
                                int64_t* row_starts, int32_t* rows, double* amounts,
                                int64_t capacity, mi_devop_point_violations* summaries);
  int (*bound_infeasible_panel_from)(mi_devop* h, const double* base_lb, const double* base_ub,
                                     int k, const int64_t* starts, const int32_t* cols,
                                     const double* new_lbs, const double* new_ubs,
                                     const double* row_lb, const double* row_ub,
                                     double tolerance, int64_t* row_starts, int32_t* rows,
                                     double* amounts, int64_t capacity,
                                     mi_devop_point_violations* summaries);
  /* DeviceLp::LastBoundRanges: the last of the four calls above. bytes_down:
   * 12 kept + 32 k with lists, 24 k for summaries only; overrides_up_bytes:
   * 16 n + 20 overrides + 8 (k + 1) for the override forms. */
  int (*last_bound_ranges)(mi_devop* h, mi_devop_row_violations* out);
  /* Appended after last_bound_ranges. DeviceLp::BoundImpliedPanel (the rule:
   * include/mi_lp.h mi_lp_bound_implied_bounds). lbs / ubs and new_lbs /
   * new_ubs: k x n; row_lb / row_ub: m each, not NULL, no NaN (checked here).
   * MILP_IMPLIED_COLUMNS = short | long | auto chooses the kernel shape. */
  int (*bound_implied_panel)(mi_devop* h, const double* lbs, const double* ubs, int k,
                             const double* row_lb, const double* row_ub, double* new_lbs,
                             double* new_ubs);
  /* The sets and their checks as bound_ranges_panel_from. */
  int (*bound_implied_panel_from)(mi_devop* h, const double* base_lb, const double* base_ub,
                                  int k, const int64_t* starts, const int32_t* cols,
                                  const double* ov_lbs, const double* ov_ubs,
                                  const double* row_lb, const double* row_ub, double* new_lbs,
                                  double* new_ubs);
  /* DeviceLp::BoundTightenedPanel in one call. tolerance finite and >= 0
   * (checked here). col_starts: k + 1; cols / new_lbs / new_ubs: `capacity`
   * entries; summaries: k, or NULL. col_starts == NULL selects summaries only.
   * A result of more than `capacity` entries returns MI_DEVOP_CAPACITY
   * (last_error says how many) with every output unwritten; it is no device
   * error. */
  int (*bound_tightened_panel)(mi_devop* h, const double* lbs, const double* ubs, int k,
                               const double* row_lb, const double* row_ub, double tolerance,
                               int64_t* col_starts, int32_t* cols, double* new_lbs,
                               double* new_ubs, int64_t capacity,
                               mi_devop_point_violations* summaries);
  int (*bound_tightened_panel_from)(mi_devop* h, const double* base_lb, const double* base_ub,
                                    int k, const int64_t* starts, const int32_t* cols_in,
                                    const double* ov_lbs, const double* ov_ubs,
                                    const double* row_lb, const double* row_ub,
                                    double tolerance, int64_t* col_starts, int32_t* cols,
                                    double* new_lbs, double* new_ubs, int64_t capacity,
                                    mi_devop_point_violations* summaries);
  int (*last_bound_implied)(mi_devop* h, mi_devop_bound_implied* out);
  /* Appended after last_bound_implied. DeviceLp::BoundPropagatePanel (the
   * rule: include/mi_lp.h mi_lp_bound_propagate). lbs / ubs and new_lbs /
   * new_ubs: k x n; row_lb / row_ub as bound_implied_panel; params checked
   * here; summaries: k, not NULL. */
  int (*bound_propagate_panel)(mi_devop* h, const double* lbs, const double* ubs, int k,
                               const mi_devop_propagate_params* params, const double* row_lb,
                               const double* row_ub, double* new_lbs, double* new_ubs,
                               mi_devop_propagation* summaries);
  /* The sets and their checks as bound_ranges_panel_from. */
  int (*bound_propagate_panel_from)(mi_devop* h, const double* base_lb, const double* base_ub,
                                    int k, const int64_t* starts, const int32_t* cols,
                                    const double* ov_lbs, const double* ov_ubs,
                                    const mi_devop_propagate_params* params,
                                    const double* row_lb, const double* row_ub, double* new_lbs,
                                    double* new_ubs, mi_devop_propagation* summaries);
  /* DeviceLp::BoundPropagatedColumnsFrom in one call. col_starts, cols,
   * new_lbs, new_ubs and capacity as bound_tightened_panel_from,
   * MI_DEVOP_CAPACITY included; summaries: k, or NULL. */
  int (*bound_propagated_columns_from)(mi_devop* h, const double* base_lb, const double* base_ub,
                                       int k, const int64_t* starts, const int32_t* cols_in,
                                       const double* ov_lbs, const double* ov_ubs,
                                       const mi_devop_propagate_params* params,
                                       const double* row_lb, const double* row_ub,
                                       int64_t* col_starts, int32_t* cols, double* new_lbs,
                                       double* new_ubs, int64_t capacity,
                                       mi_devop_propagation* summaries);
  int (*last_bound_propagate)(mi_devop* h, mi_devop_bound_propagate* out);
  /* Appended after last_bound_propagate. DeviceLp::ColumnPenaltiesPanel (the
   * rule: include/mi_lp.h mi_lp_row_penalties). y: k x m; d, status: N; unit:
   * N, or NULL; down_dist, up_dist: k; out: k records. The arguments are
   * checked here as mi_lp_row_penalties checks them: a bad one is an error
   * with nothing written and no device error. */
  int (*column_penalties_panel)(mi_devop* h, const double* y, int k, const double* d,
                                const int8_t* status, const double* unit,
                                const double* down_dist, const double* up_dist,
                                double pivot_tolerance, mi_devop_branch_penalty* out);
  int (*last_penalties)(mi_devop* h, mi_devop_penalties* out);
  /* Appended after last_penalties. DeviceLp::ColumnCutsPanel (the rule:
   * include/mi_lp.h mi_lp_row_gomory_cuts). y: k x m; status: N; unit: N, or
   * NULL; f0, row_unit: k. row_starts: k + 1, or NULL (summaries alone: cols
   * and vals are not touched); cols, vals: capacity entries; summaries: k, or
   * NULL. A result of more than `capacity` entries returns MI_DEVOP_CAPACITY
   * with nothing written. The arguments are checked here as
   * mi_lp_row_gomory_cuts checks them: a bad one is an error with nothing
   * written and no device error. */
  int (*column_cuts_panel)(mi_devop* h, const double* y, int k, const int8_t* status,
                           const double* unit, const double* f0, const double* row_unit,
                           double zero_tolerance, double drop_tolerance, int64_t* row_starts,
                           int32_t* cols, double* vals, int64_t capacity,
                           mi_devop_cut_summary* summaries);
  int (*last_cuts)(mi_devop* h, mi_devop_cuts* out);
  /* Appended after last_cuts. The device triangular solves (engine/
   * device_solver.h) on a TriangularMatrix owned by the handle; the handle's
   * own [A | I] plays no part (it may be 1 x 1).
   *
   * tri_set_matrix builds the matrix with Reset and AddTriangularColumn:
   * column c holds the entries [col_starts[c], col_starts[c + 1]) of rows /
   * vals in the caller's order (none of them on row c) and the diagonal
   * diag[c]; the first non-identity column and the unit-diagonal flag come out
   * as the class computes them. Checked here: n >= 1, col_starts[0] == 0,
   * monotone starts, rows in [0, n) and off the diagonal. NOT checked, the
   * caller's precondition: the matrix is triangular for the kinds it is
   * solved with (rows > column for MI_DEVOP_TRI_UPPER_T, _LOWER, _LOWER_T and
   * _UNIT_ROW; rows < column for _UPPER_T_UP and _UPPER) and no diagonal is
   * zero. */
  int (*tri_set_matrix)(mi_devop* h, int n, const int64_t* col_starts, const int32_t* rows,
                        const double* vals, const double* diag);
  /* DeviceLp::Solve. kind: MI_DEVOP_TRI_*; key != 0 names the matrix (a new
   * key rebuilds the schedule); x: n values in and out, untouched when
   * *on_device == 0. start is the engine's argument of LowerSolveStartingAt:
   * every x below it must be zero (the engine's own precondition, not
   * checked). */
  int (*tri_solve)(mi_devop* h, int kind, uint64_t key, int start, double* x, int* on_device);
  /* DeviceLp::SolvePair; both vectors untouched when *on_device == 0. */
  int (*tri_solve_pair)(mi_devop* h, int kind, uint64_t key, double* x0, double* x1,
                        int* on_device);
  /* DeviceLp::StartAsyncU / FinishAsyncU / DropAsyncU. finish: x holds the
   * vector given to begin and receives the result; without a begin before it
   * it is an error. */
  int (*tri_async_begin)(mi_devop* h, uint64_t key, const double* x, int* started);
  int (*tri_async_finish)(mi_devop* h, double* x);
  int (*tri_async_drop)(mi_devop* h);
  /* The host loop of the kind on the same matrix (engine/lu.h):
   * TransposeLowerSolve (_UPPER_T, _LOWER_T), TransposeUpperSolve
   * (_UPPER_T_UP), LowerSolveStartingAt(start) (_LOWER, _UNIT_ROW), UpperSolve
   * (_UPPER). */
  int (*tri_host_solve)(mi_devop* h, int kind, int start, double* x);
  /* DeviceLp::LastTri: the last tri_solve, tri_solve_pair or tri_async_begin. */
  int (*last_tri)(mi_devop* h, mi_devop_tri* out);
  /* The level widths of the schedule last_tri describes: *count of them, the
   * first min(*count, capacity) written to widths. */
  int (*last_tri_level_widths)(mi_devop* h, int32_t* widths, int capacity, int* count);
} mi_devop_api;

extern const mi_devop_api mi_devop_table;

/* The matrix entries, in a table of their own behind mi_devop_table (whose
 * length tests/test_tri_ref_cpu.py pins): mi_devop_matrix_table. */
typedef struct mi_devop_matrix_api {
  /* k rows as lists (include/mi_lp.h mi_lp_add_rows; checked here as that
   * call checks them) extend the handle's csc / csr on the host
   * (CompactSparseMatrix::AppendRows, AppendTransposedRows) and the device
   * with DeviceLp::AppendRows. The relevant mask the handle remembers is all
   * ones afterwards, as after create. */
  int (*append_rows)(mi_devop* h, int k, const int64_t* row_starts, const int32_t* cols,
                     const double* vals);
  /* The matrix as the device holds it: CSC starts (N + 1) / rows / vals (nnz
   * each), CSR starts (m + 1) / cols / vals, *nd dense columns in dense_cols
   * (room for n), and the dense block in dense_block (body then tail, nd * m
   * values; more than `capacity` returns MI_DEVOP_CAPACITY with only *nd
   * written). */
  int (*fetch_matrix)(mi_devop* h, int64_t* starts, int32_t* rows, double* vals,
                      int64_t* t_starts, int32_t* t_cols, double* t_vals, int32_t* nd,
                      int32_t* dense_cols, double* dense_block, int64_t capacity);
  int (*last_append)(mi_devop* h, mi_devop_append* out);
} mi_devop_matrix_api;

extern const mi_devop_matrix_api mi_devop_matrix_table;

/* DeviceLp::LastDelete: the last delete_rows. The shapes are MI_DEVOP_MOVE_*
 * bits, per thread and per workgroup, for the CSC columns and the CSR rows. */
typedef struct mi_devop_delete {
  int32_t path;          /* 1 compacted on the device, 2 full upload */
  int32_t rows;          /* deleted rows */
  int64_t entries;       /* structural entries removed */
  int64_t bytes_up;      /* host -> device for the matrix */
  int32_t column_shapes; /* of the count and move kernels that ran for columns */
  int32_t row_shapes;    /* of the move kernels that ran for rows */
  double device_ms;      /* the mask's copy and the kernels, by events */
} mi_devop_delete;

/* Row deletion, in a third table: mi_devop_matrix_delete_table. */
typedef struct mi_devop_matrix_delete_api {
  /* The rows of delete_mask (m bytes, non-zero deletes; include/mi_lp.h
   * mi_lp_delete_rows) leave the handle's csc / csr on the host
   * (CompactSparseMatrix::DeleteRows, DeleteTransposedRows) and the device
   * with DeviceLp::DeleteRows. The relevant mask the handle remembers is all
   * ones afterwards, as after create. */
  int (*delete_rows)(mi_devop* h, const uint8_t* delete_mask);
  int (*last_delete)(mi_devop* h, mi_devop_delete* out);
} mi_devop_matrix_delete_api;

extern const mi_devop_matrix_delete_api mi_devop_matrix_delete_table;

#ifdef __cplusplus
}
#endif

#endif /* MI_LP_DEVOP_H_ */
