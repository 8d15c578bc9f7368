/*
 * mi_lp.h -- C ABI of the MI355X revised-simplex LP engine (drop-in for Glop).
 *
 * Plain pointers and sizes only; no C++ or torch types cross this boundary.
 * Every entry point below replaces one piece of the Glop / MPSolver interface
 * of OR-Tools 9.7 (paths relative to the reference checkout):
 *
 *   mi_lp_create / mi_lp_destroy     glop::RevisedSimplex ctor/dtor
 *                                    (ortools/glop/revised_simplex.h:125-129)
 *   mi_lp_set_params                 RevisedSimplex::SetParameters
 *                                    (revised_simplex.h:132, .cc:3586-3593)
 *   mi_lp_load                       the LinearProgram handed to Solve()
 *                                    (revised_simplex.cc:139, lp_data.h:56);
 *                                    CSC, rows sorted per column, no explicit
 *                                    zeros (LinearProgram::IsCleanedUp,
 *                                    lp_solver.cc:185-191)
 *   mi_lp_load_basis_state           RevisedSimplex::LoadStateForNextSolve
 *                                    (revised_simplex.h:153, .cc:120-124)
 *   mi_lp_clear_basis_state          RevisedSimplex::ClearStateForNextSolve (.cc:114)
 *   mi_lp_notify_matrix_unchanged    NotifyThatMatrixIsUnchangedForNextSolve (.cc:131)
 *   mi_lp_solve                      RevisedSimplex::Solve (revised_simplex.cc:139-635)
 *                                    + the ProblemStatus mapping of
 *                                    LPSolver::RunRevisedSimplexIfNeeded
 *                                    (lp_solver.cc:591-658)
 *   mi_lp_get_*                      GetVariableValue / GetReducedCost /
 *                                    GetDualValue / GetConstraintActivity /
 *                                    GetVariableStatus / GetConstraintStatus /
 *                                    GetBasis / GetState / GetPrimalRay /
 *                                    GetDualRay / GetDualRayRowCombination
 *                                    (revised_simplex.h:172-239, .cc:637-713)
 *   mi_lp_begin / mi_lp_run_until /  the PrimalMinimize/DualMinimize loops
 *   mi_lp_finish                     (revised_simplex.cc:2751-3367) driven in
 *                                    bounded slices (benchmark harness only)
 *   mi_lp_batch_solve                CP-SAT's per-worker LP call-out
 *                                    (sat/linear_programming_constraint.cc:709-760)
 *                                    for many independent LPs at once
 *
 * Error codes mirror glop::Status::ErrorCode (ortools/glop/status.h:29-44).
 * Threading: one handle = one host thread = one HIP stream (RevisedSimplex is
 * not thread safe either).
 */
#ifndef MI_LP_H_
#define MI_LP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Opaque solver handle (one glop::RevisedSimplex + its device state). */
typedef struct mi_lp mi_lp;

/* glop::Status::ErrorCode (status.h:29-44) + ABI-level codes. */
enum {
  MI_LP_OK = 0,
  MI_LP_ERROR_LU = 1,
  MI_LP_ERROR_BOUND = 2,
  MI_LP_ERROR_NULL = 3,
  MI_LP_ERROR_INVALID_PROBLEM = 4,
  MI_LP_ERROR_DEVICE = 100, /* HIP runtime failure or missing GPU */
  MI_LP_ERROR_STATE = 101,  /* call out of order (e.g. getter before solve) */
  MI_LP_ERROR_INTERNAL = 102 /* host exception inside the engine (e.g. out of
                                memory); the handle stays usable */
};

/* glop::ProblemStatus (ortools/lp_data/lp_types.h:106-168). */
enum {
  MI_LP_OPTIMAL = 0,
  MI_LP_PRIMAL_INFEASIBLE = 1,
  MI_LP_DUAL_INFEASIBLE = 2,
  MI_LP_INFEASIBLE_OR_UNBOUNDED = 3,
  MI_LP_PRIMAL_UNBOUNDED = 4,
  MI_LP_DUAL_UNBOUNDED = 5,
  MI_LP_INIT = 6,
  MI_LP_PRIMAL_FEASIBLE = 7,
  MI_LP_DUAL_FEASIBLE = 8,
  MI_LP_ABNORMAL = 9,
  MI_LP_INVALID_PROBLEM = 10,
  MI_LP_IMPRECISE = 11
};

/* glop::VariableStatus / ConstraintStatus (lp_types.h:188-219). */
enum {
  MI_LP_BASIC = 0,
  MI_LP_FIXED_VALUE = 1,
  MI_LP_AT_LOWER_BOUND = 2,
  MI_LP_AT_UPPER_BOUND = 3,
  MI_LP_FREE = 4
};

/* GlopParameters enums (ortools/glop/parameters.proto:49-92). */
enum { MI_LP_DANTZIG = 0, MI_LP_STEEPEST_EDGE = 1, MI_LP_DEVEX = 2 };
enum { MI_LP_BASIS_NONE = 0, MI_LP_BASIS_BIXBY = 1, MI_LP_BASIS_TRIANGULAR = 2,
       MI_LP_BASIS_MAROS = 3 };

/* POD mirror of the GlopParameters fields read by RevisedSimplex
 * (ortools/glop/parameters.proto, field numbers in comments). Fill with
 * mi_glop_params_default() first; defaults are the proto defaults. */
typedef struct mi_glop_params {
  int32_t use_dual_simplex;                          /* 31, false  */
  int32_t feasibility_rule;                          /* 1, STEEPEST_EDGE */
  int32_t optimization_rule;                         /* 2, STEEPEST_EDGE */
  int32_t initial_basis;                             /* 17, TRIANGULAR */
  int32_t use_transposed_matrix;                     /* 18, true */
  int32_t basis_refactorization_period;              /* 19, 64 */
  int32_t dynamically_adjust_refactorization_period; /* 63, true */
  int32_t change_status_to_imprecise;                /* 58, true */
  int32_t markowitz_zlatev_parameter;                /* 29, 3 */
  int32_t allow_simplex_algorithm_change;            /* 32, false */
  int32_t devex_weights_reset_period;                /* 33, 150 */
  int32_t use_middle_product_form_update;            /* 35, true; false = product-form etas
                                                        (async/inline tau off) */
  int32_t initialize_devex_with_column_norms;        /* 36, true */
  int32_t exploit_singleton_column_in_initial_basis; /* 37, true */
  int32_t random_seed;                               /* 43, 1 */
  int32_t perturb_costs_in_dual_simplex;             /* 53, false */
  int32_t use_dedicated_dual_feasibility_algorithm;  /* 62, true */
  int32_t push_to_vertex;                            /* 65, true */
  int32_t dual_price_prioritize_norm;                /* 69, false */
  int32_t use_scaling;                               /* 16, true (Bixby only) */
  int64_t max_number_of_iterations;                  /* 27, -1 */
  double refactorization_threshold;                  /* 6, 1e-9 */
  double recompute_reduced_costs_threshold;          /* 8, 1e-8 */
  double recompute_edges_norm_threshold;             /* 9, 100 */
  double primal_feasibility_tolerance;               /* 10, 1e-8 */
  double dual_feasibility_tolerance;                 /* 11, 1e-8 */
  double ratio_test_zero_threshold;                  /* 12, 1e-9 */
  double harris_tolerance_ratio;                     /* 13, 0.5 */
  double small_pivot_threshold;                      /* 14, 1e-6 */
  double minimum_acceptable_pivot;                   /* 15, 1e-6 */
  double drop_tolerance;                             /* 52, 1e-14 */
  double solution_feasibility_tolerance;             /* 22, 1e-6 */
  double max_number_of_reoptimizations;              /* 56, 40 */
  double lu_factorization_pivot_threshold;           /* 25, 0.01 */
  double max_time_in_seconds;                        /* 26, inf */
  double max_deterministic_time;                     /* 45, inf */
  double markowitz_singularity_threshold;            /* 30, 1e-15 */
  double dual_small_pivot_threshold;                 /* 38, 1e-4 */
  double objective_lower_limit;                      /* 40, -inf */
  double objective_upper_limit;                      /* 41, inf */
  double degenerate_ministep_factor;                 /* 42, 0.01 */
  double relative_cost_perturbation;                 /* 54, 1e-5 */
  double relative_max_cost_perturbation;             /* 55, 1e-7 */
  double initial_condition_number_threshold;         /* 59, 1e50 */
  double crossover_bound_snapping_distance;          /* 64, inf */
} mi_glop_params;

typedef struct mi_lp_result {
  int32_t problem_status; /* MI_LP_OPTIMAL ... */
  int32_t error_code;     /* MI_LP_OK ... (non-OK => problem_status ABNORMAL) */
  int64_t iterations;     /* RevisedSimplex::GetNumberOfIterations */
  double objective;       /* RevisedSimplex::GetObjectiveValue */
  double deterministic_time;
  double solve_seconds;   /* wall time of Solve() */
} mi_lp_result;

/* Per-kernel accounting kept by the engine (roofline bookkeeping). */
typedef struct mi_lp_kernel_stats {
  int64_t launches[16];
  double algorithmic_bytes[16];
  double device_ms[16]; /* HIP-event time, filled when timing is enabled */
  double call_ms[16];   /* host wall time of the whole device call: uploads,
                           launches, downloads, synchronization */
} mi_lp_kernel_stats;

enum {
  MI_K_PRICING = 0,     /* ComputeReducedCosts SpMV (reduced_costs.cc:352-423) */
  MI_K_UPDATE_ROW = 1,  /* UpdateRow column/row-wise (update_row.cc:196-306) */
  MI_K_PRIMAL_NORMS = 2,/* UpdateEdgeSquaredNorms (primal_edge_norms.cc:208-258) */
  MI_K_RC_UPDATE = 3,   /* UpdateReducedCosts (reduced_costs.cc:444-488) */
  MI_K_TRI_SOLVE = 4,   /* dense U solve of FTRAN, TriangularMatrix::TransposeLowerSolve
                           (sparse.cc:899-955, lu_factorization.cc:314-331) */
  MI_K_COL_NORMS = 5,   /* initial edge norms, identity basis (primal_edge_norms.cc:147-161) */
  MI_K_SPMV_ROWS = 6,   /* A x row sums: residual / basic values (variable_values.cc:101-133) */
  MI_K_SINGLE_ROW = 7,  /* ComputeUpdatesForSingleRow (update_row.cc:261-280) */
  MI_K_DUAL_RATIO = 8,  /* dual ratio-test candidate filter (entering_variable.cc:37-130) */
  MI_K_READBACK = 9,    /* update-row list download / single-coefficient reads */
  MI_K_TRI_SOLVE_TAU = 10, /* the same dense U solve for the tau FTRAN on the
                              factorization's worker thread (dual_edge_norms.cc:134-141) */
  MI_K_TRI_SOLVE_L = 11,   /* dense L solve of FTRAN (sparse.cc:793-812) on the device */
  MI_K_TRI_SOLVE_T = 12,   /* dense solves of BTRAN on the device: U^T (TransposeUpperSolve,
                              sparse.cc:848-897), L^T (TransposeLowerSolve), the unit-row U^T
                              (LowerSolveStartingAt, lu_factorization.cc:405-436) */
  MI_K_TRI_SOLVE_UPPER = 13, /* dense UpperSolve (sparse.cc:814-846): the product-form and
                                squared-norm FTRANs' U */
  MI_K_SDUAL = 14,      /* device dual simplex segment: whole phase-II dual iterations of one
                           LP on one workgroup (revised_simplex.cc:3058-3367); bytes = the
                           state arena moved in and out */
  MI_K_EXCHANGE = 15,   /* cross-process split joins (mi_lp_set_exchange): all-gathers, host
                           wall time, bytes gathered */
  MI_K_COUNT = 16
};

void mi_glop_params_default(mi_glop_params* p);

/* Returns the number of visible GPUs (0 on a host without one). */
int mi_lp_device_count(void);
/* Process teardown: drains the persistent batched-segment grids and joins the
 * engine's service threads (LU servers, batched-launch launchers) while the
 * HIP runtime is still up. Registered with atexit when the first such object
 * is created; hosts whose own teardown runs earlier (Python atexit, a plugin
 * unload) call it explicitly. Idempotent; later solves restart what they need.
 * (No Glop counterpart: Glop owns no threads or device state.) */
int mi_lp_shutdown(void);

int mi_lp_create(int device, mi_lp** out);
int mi_lp_destroy(mi_lp* h);
const char* mi_lp_last_error(const mi_lp* h);
int mi_lp_set_params(mi_lp* h, const mi_glop_params* p);

/* m constraints, n variables; A in CSC with n+1 col_starts. Bounds may be
 * +/-INFINITY. maximize != 0 => objective is maximized. */
int mi_lp_load(mi_lp* h, int32_t m, int32_t n, const int64_t* col_starts,
               const int32_t* row_idx, const double* vals, const double* col_lb,
               const double* col_ub, const double* row_lb, const double* row_ub,
               const double* obj, double obj_offset, double obj_scale,
               int32_t maximize);

/* Appends k rows to the loaded LP (the cuts of a cut loop). The rows are lists,
 * the shape mi_lp_get_cut_rows returns: row j holds (cols[p], vals[p]) for p in
 * [row_starts[j], row_starts[j + 1]), row_starts has k + 1 entries, and per
 * row the structural columns are strictly ascending in [0, n), the
 * coefficients finite and non-zero; row_lb / row_ub may be +/-INFINITY (a
 * Gomory cut is row_lb = rhs, row_ub = +INFINITY). Row j becomes row m + j and
 * its slack column n + m + j; old columns and old slacks keep their indices.
 *
 * The contract: in any sequence of calls on a handle, replacing
 * mi_lp_add_rows(R) by mi_lp_load of the extended LP (the same columns, each
 * with R's entries appended, and the handle's current column bounds,
 * objective, offset, scale and sense) changes no bit of anything the handle
 * later returns: solve results, iterations, basis, state and rays, every panel
 * call (refused until the next solve, as after a load),
 * mi_lp_batch_solve_bounds (the matrix fingerprint is that of the load) and
 * the stores of the mi_lp_get_* lists (forgotten, as on a load). That holds
 * before a first solve, after mi_lp_load_basis_state, for two appends in a
 * row, and for a mi_lp_load between an append and the solve. Only the time
 * and the bytes moved differ: where the handle's matrix is resident on the
 * device (it has been solved since its last load), only the new rows cross
 * PCIe, they are merged into the resident CSC and CSR on the device, and the
 * next solve takes the warm new-rows path of
 * RevisedSimplex::Initialize (revised_simplex.cc:1334-1565) without the
 * entry-by-entry compare, the host rebuild or the upload. The host still
 * shifts its own columns and re-hashes A (one pass each). One exception to
 * the contract: after mi_lp_notify_matrix_unchanged the load twin would
 * solve on the stale matrix; the append is honoured instead.
 *
 * k = 0 succeeds and is the load of the same LP.
 *
 *   MI_LP_ERROR_NULL             h or row_starts NULL; cols or vals NULL with
 *                                row_starts[k] > 0; row_lb or row_ub NULL with
 *                                k > 0
 *   MI_LP_ERROR_STATE            before mi_lp_load, or while a begun solve runs
 *   MI_LP_ERROR_INVALID_PROBLEM  k < 0; row_starts[0] != 0 or decreasing
 *                                row_starts; a column out of range or not
 *                                strictly ascending; a zero, NaN or infinite
 *                                coefficient; a NaN bound; n + m + k past
 *                                int32 or nnz + e + m + k past int64
 * On every error nothing changes, neither on the host nor on the device. */
typedef struct mi_lp_append_info {
  int32_t path;      /* 0: no device matrix yet (host only); 1: merged on the device;
                        2: full upload from the extended host matrices (column
                        shards, or 32768 rows and more) */
  int32_t rows;      /* k */
  int64_t entries;   /* e = row_starts[k] */
  int64_t bytes_up;  /* bytes sent host -> device by this call for the matrix:
                        on path 1 at most 12 (e + k) + 8 k */
} mi_lp_append_info;
int mi_lp_add_rows(mi_lp* h, int32_t k, const int64_t* row_starts, const int32_t* cols,
                   const double* vals, const double* row_lb, const double* row_ub,
                   mi_lp_append_info* info /* may be NULL */);

/* Deletes rows from the loaded LP (the cuts a cut loop purges, CP-SAT's
 * LinearConstraintManager::ChangeLp over glop's LinearProgram::DeleteRows).
 * delete_mask has m bytes; a non-zero byte deletes its row. Kept rows keep
 * their order: row r becomes row r - (deleted rows below r) and its slack
 * column n + that index; the slack columns of deleted rows disappear;
 * structural columns keep their indices.
 *
 * The contract: in any sequence of calls on a handle, mi_lp_delete_rows(mask)
 * may be replaced by (1) mi_lp_load of the reduced LP (the same columns with
 * the deleted rows' entries removed and the rows renumbered, the kept row
 * bounds, and the handle's current column bounds, objective, offset, scale
 * and sense) and (2), only if the state the next solve would start from (the
 * last solve's final state, or the one given to mi_lp_load_basis_state since)
 * is non-empty and has n + m entries, mi_lp_load_basis_state of that state
 * with the entries n + r of the deleted rows removed; a state of another
 * length, or none, means (1) alone. No bit of anything the handle later
 * returns changes: solve results, iterations, basis, state and rays, every
 * panel call (refused until the next solve, as after a load),
 * mi_lp_batch_solve_bounds (the matrix fingerprint is that of the load) and
 * the stores of the mi_lp_get_* lists (forgotten, as on a load).
 * mi_lp_set_starting_variable_values is left as the load leaves it. That
 * holds before a first solve, after mi_lp_load_basis_state, for two deletes
 * in a row, for a delete after an append (of exactly the appended rows too),
 * for an append after a delete (of as many rows too), and for a mi_lp_load
 * between the delete and the solve. Only the time and the bytes moved
 * differ: where the handle's matrix is resident on the device, only the mask
 * crosses PCIe, the resident CSC and CSR are compacted on the device, and the
 * next solve starts without the entry-by-entry compare, the host rebuild or
 * the upload (it refactorizes, as glop does). The host still compacts its own
 * columns and re-hashes A (one pass each), and until the next solve it keeps
 * a copy of the last solve's matrix if one of that solve's rows went. One
 * exception to the contract: after mi_lp_notify_matrix_unchanged the load
 * twin would solve on the stale matrix; the delete is honoured instead.
 *
 * A mask with no row set succeeds and is the load of the same LP, with (2)
 * still applied. A mask that deletes every row is the load of the LP with
 * m = 0; it takes the full upload (path 2), never the compaction.
 *
 *   MI_LP_ERROR_NULL   h NULL, or delete_mask NULL with m > 0
 *   MI_LP_ERROR_STATE  before mi_lp_load, or while a begun solve runs
 * There is no MI_LP_ERROR_INVALID_PROBLEM case. On every error nothing
 * changes, neither on the host nor on the device. */
typedef struct mi_lp_delete_info {
  int32_t path;      /* 0: no device matrix yet (host only); 1: compacted on the
                        device; 2: full upload from the reduced host matrices
                        (column shards, or no row kept) */
  int32_t rows;      /* d = deleted rows */
  int64_t entries;   /* structural entries removed */
  int64_t bytes_up;  /* host -> device for the matrix: on path 1 the mask, m bytes */
} mi_lp_delete_info;
int mi_lp_delete_rows(mi_lp* h, const uint8_t* delete_mask /* m; non-zero deletes */,
                      mi_lp_delete_info* info /* may be NULL */);

/* statuses: n+m glop::VariableStatus values (structural then slacks). */
int mi_lp_load_basis_state(mi_lp* h, const int8_t* statuses, int32_t len);
int mi_lp_clear_basis_state(mi_lp* h);
/* Replaces the variable bounds of the loaded LP (n each); the matrix stays
 * resident in HBM. LinearProgram::SetVariableBounds as CP-SAT does before
 * each LP solve (sat/linear_programming_constraint.cc:412, 512, 535, 705). */
int mi_lp_set_variable_bounds(mi_lp* h, const double* col_lb, const double* col_ub);
int mi_lp_notify_matrix_unchanged(mi_lp* h);

/* CP-SAT's calls on the RevisedSimplex it keeps per LP constraint
 * (sat/linear_programming_constraint.cc:319,430,1247,1264):
 *   mi_lp_notify_matrix_changed          NotifyThatMatrixIsChangedForNextSolve
 *                                        (revised_simplex.h:169, .cc:135)
 *   mi_lp_set_starting_variable_values   SetStartingVariableValuesForNextSolve
 *                                        (revised_simplex.h:161, .cc:126); n+m values
 *   mi_lp_set_integrality_scale          SetIntegralityScale (revised_simplex.h:237,
 *                                        .cc:2588); a later OPTIMAL solve then runs
 *                                        Polish() (.cc:341-344, 2595-2734)
 *   mi_lp_objective_limit_reached        objective_limit_reached (revised_simplex.h:186)
 *   mi_lp_get_unit_row_left_inverse      GetUnitRowLeftInverse (revised_simplex.h:209):
 *                                        e_row^T B^-1 of the current basis, m dense
 *                                        values + its non-zero rows (non_zeros may be
 *                                        NULL; an empty list means "dense")
 *   mi_lp_compute_dictionary /           ComputeDictionary (revised_simplex.h:226,
 *   mi_lp_get_dictionary                 .cc:3785): B^-1 A row by row, scaled by
 *                                        column_scales (NULL: unscaled); the first call
 *                                        returns the entry count, the second copies
 *                                        row_starts (m+1), cols and values out. */
int mi_lp_notify_matrix_changed(mi_lp* h);
int mi_lp_set_starting_variable_values(mi_lp* h, const double* values, int32_t len);
int mi_lp_set_integrality_scale(mi_lp* h, int32_t col, double scale);
/* RevisedSimplex::ClearIntegralityScales (revised_simplex.h:236), called by
 * sat/linear_programming_constraint.cc:424 before it sets the scales again. */
int mi_lp_clear_integrality_scales(mi_lp* h);
int mi_lp_objective_limit_reached(const mi_lp* h, int32_t* reached);
int mi_lp_get_unit_row_left_inverse(mi_lp* h, int32_t row, double* values, int32_t* non_zeros,
                                    int32_t* num_non_zeros);
int mi_lp_compute_dictionary(mi_lp* h, const double* column_scales, int32_t scales_len,
                             int64_t* nnz);
int mi_lp_get_dictionary(const mi_lp* h, int64_t* row_starts, int32_t* cols, double* values);

/* Several rows of rho^T [A | I] in one call that reads A once per panel of up
 * to 16 vectors (what a cut loop otherwise computes on the host, one row at a
 * time, after sat/linear_programming_constraint.cc:1247). No Glop call does
 * this; each result is defined by two pieces of Glop's public surface:
 *   mi_lp_row_combinations               out[j (n+m) + col] = dot(col, y_j) for j < k
 *                                        and EVERY column col of [A | I], where dot is
 *                                        CompactSparseMatrix::ColumnScalarProduct
 *                                        (sparse.h:514-542): four accumulators over the
 *                                        column's entries in groups of four from +0.0,
 *                                        ((r1 + r2) + r3) + r4, then the <= 3 tail terms
 *                                        in order, every product and sum rounded
 *                                        separately. An empty column gives +0.0, a slack
 *                                        column 0.0 + y[r]. The full row over all n+m
 *                                        columns, unfiltered: no relevant mask, no drop
 *                                        tolerance, no cost term. Changes no state a
 *                                        later solve reads.
 *   mi_lp_get_tableau_rows               the same with y_j = the values of
 *                                        GetUnitRowLeftInverse(rows[j])
 *                                        (revised_simplex.h:209) of the current basis,
 *                                        computed by k host left solves in the caller's
 *                                        order; left_inverses (k x m, may be NULL)
 *                                        receives them. Side effects: exactly those of k
 *                                        mi_lp_get_unit_row_left_inverse calls.
 * y: k x m, out: k x (n+m), both vector-major. k = 0 writes nothing and
 * succeeds; k < 0 or a row outside [0, m) is MI_LP_ERROR_INVALID_PROBLEM with
 * nothing written; other errors as mi_lp_get_unit_row_left_inverse. */
int mi_lp_row_combinations(mi_lp* h, const double* y, int32_t k, double* out);
/* rows: k basic row indices. out: k x (n+m). left_inverses: k x m, or NULL. */
int mi_lp_get_tableau_rows(mi_lp* h, const int32_t* rows, int32_t k, double* out,
                           double* left_inverses);

/* The same rows as sparse (column, value) lists, filtered and packed on the
 * GPU so that only the kept entries come back (a cut loop keeps the non-basic
 * and/or structural columns above a drop tolerance). Two calls, as
 * mi_lp_compute_dictionary / mi_lp_get_dictionary:
 *   mi_lp_row_combinations_sparse        computes the k rows, stores them in the handle
 *   mi_lp_get_tableau_rows_sparse        and writes row_starts (k+1; row_starts[k] is the
 *                                        entry count). Row j holds, in strictly increasing
 *                                        column order, every column col of [A | I] that
 *                                        (a) passes column_filter: MI_LP_COLUMNS_STRUCTURAL
 *                                        means col < n, MI_LP_COLUMNS_NON_BASIC means the
 *                                        column's status in mi_lp_get_state is not
 *                                        MI_LP_BASIC, both bits mean both, 0 every column;
 *                                        and (b) has fabs(v) > drop_tolerance, where v is
 *                                        bit for bit out[j (n+m) + col] of the dense call
 *                                        above. The comparison is strict (update_row.cc's
 *                                        fabs(acc) > drop_tolerance): at tolerance 0 both
 *                                        +0.0 and -0.0 are dropped, a NaN result is
 *                                        dropped, +-inf results are kept, and
 *                                        drop_tolerance = +inf gives empty rows.
 *   mi_lp_get_sparse_rows                copies the stored cols and vals out,
 *                                        row_starts[k] of each. The stored result lives in
 *                                        the handle until the next sparse call, mi_lp_load
 *                                        or mi_lp_destroy.
 * Errors: drop_tolerance < 0 or NaN, unknown filter bits, k < 0 or a row
 * outside [0, m): MI_LP_ERROR_INVALID_PROBLEM with nothing written and the
 * stored result untouched. NULL y, rows or row_starts: MI_LP_ERROR_NULL.
 * Before a solve: MI_LP_ERROR_STATE. mi_lp_get_sparse_rows before any sparse
 * call, or after mi_lp_load: MI_LP_ERROR_STATE. k = 0 succeeds, writes
 * row_starts[0] = 0 and stores an empty result. Side effects on solver state
 * are those of the dense calls: none for mi_lp_row_combinations_sparse, k
 * mi_lp_get_unit_row_left_inverse calls for mi_lp_get_tableau_rows_sparse. */
enum { MI_LP_COLUMNS_ALL = 0, MI_LP_COLUMNS_STRUCTURAL = 1, MI_LP_COLUMNS_NON_BASIC = 2 };
int mi_lp_row_combinations_sparse(mi_lp* h, const double* y, int32_t k, double drop_tolerance,
                                  uint32_t column_filter, int64_t* row_starts);
/* left_inverses: k x m, or NULL. */
int mi_lp_get_tableau_rows_sparse(mi_lp* h, const int32_t* rows, int32_t k,
                                  double drop_tolerance, uint32_t column_filter,
                                  int64_t* row_starts, double* left_inverses);
int mi_lp_get_sparse_rows(const mi_lp* h, int32_t* cols, double* vals);

/* The same rows reduced on the GPU to one branching penalty record each: the
 * Driebeek penalty with Tomlin's integer strengthening, the bound that the
 * first dual simplex pivot of each child of a branching gives (what a
 * branch-and-bound host ranks or drops children by before it pays for
 * mi_lp_batch_solve_bounds). Only 32 bytes per vector come down. Glop's
 * dictionary has [A | I] x = 0, so the basic variable of row r is
 * x_B(r) = -sum over non-basic j of alpha_j x_j with alpha = rho^T [A | I],
 * rho = row r of B^-1: alpha is bit for bit mi_lp_row_combinations' out for
 * y = rho.
 *   mi_lp_row_penalties                  out[v] for v < k from alpha = row v of
 *                                        mi_lp_row_combinations(y) and the caller's d
 *                                        (n+m reduced costs, minimisation sense), status
 *                                        (n+m, MI_LP_BASIC .. MI_LP_FREE), unit (n+m steps
 *                                        of integer columns in LP units, 0 for a
 *                                        continuous column; NULL: all 0), down_dist[v],
 *                                        up_dist[v] and pivot_tolerance. Per column col,
 *                                        in doubles without FMA:
 *                                        1. BASIC and FIXED_VALUE columns take no part.
 *                                        2. cost = d > 0 ? d : 0.0 AT_LOWER_BOUND,
 *                                           d < 0 ? -d : 0.0 AT_UPPER_BOUND, 0.0 FREE.
 *                                        3. A NaN alpha or d: the column takes part in both
 *                                           directions with the candidate +0.0 (a NaN only
 *                                           ever says "not proven").
 *                                        4. Else, unless fabs(alpha) > pivot_tolerance
 *                                           (strict), the column takes no part.
 *                                        5. Else it takes part in the down direction iff
 *                                           FREE, AT_LOWER_BOUND with alpha > 0 or
 *                                           AT_UPPER_BOUND with alpha < 0, and in the up
 *                                           direction iff FREE, AT_LOWER_BOUND with
 *                                           alpha < 0 or AT_UPPER_BOUND with alpha > 0
 *                                           (raising a non-basic column by t moves x_B(r)
 *                                           by -alpha t).
 *                                        6. Its candidate there is c = dist * (cost /
 *                                           fabs(alpha)); with unit > 0 then
 *                                           c = c < cost * unit ? cost * unit : c; a NaN c
 *                                           (0 * inf, inf / inf) counts as +0.0.
 *                                        Per direction: the penalty is the smallest
 *                                        candidate (+inf without one), the column the
 *                                        lowest one whose candidate equals it (-1 without
 *                                        one), the count the number of columns that take
 *                                        part. Candidates are >= +0.0, never -0.0 or NaN,
 *                                        so the record does not depend on the reduction
 *                                        order. A count of 0 proves that child infeasible.
 *                                        With unit all 0 the penalty bounds the child's LP
 *                                        objective increase (minimisation sense), with
 *                                        integer steps the child's integer problem.
 *                                        Everything is the caller's; changes no state.
 *   mi_lp_branching_penalties            the same for the k BASIC columns cols (structural
 *                                        or slack) of the current basis: y_j = the values
 *                                        of GetUnitRowLeftInverse(row of cols[j]) as in
 *                                        mi_lp_get_tableau_rows (left_inverses: k x m, or
 *                                        NULL; the same side effects); status =
 *                                        mi_lp_get_state's; d in the simplex's internal
 *                                        minimisation sense: for a minimised LP
 *                                        d[col] = mi_lp_get_reduced_costs[col] (col < n)
 *                                        and d[n + r] = -mi_lp_get_duals[r]; for a
 *                                        maximised LP the solver minimises -objective and
 *                                        the getters return the negated internal values,
 *                                        so d[col] = -mi_lp_get_reduced_costs[col] and
 *                                        d[n + r] = +mi_lp_get_duals[r], and the penalties
 *                                        bound the DECREASE of the maximised objective.
 *                                        NULL down_dist / up_dist mean v - floor(v) and
 *                                        ceil(v) - v of the column's current value v
 *                                        (mi_lp_get_primal; for the slack of row r,
 *                                        -mi_lp_get_activities[r]). unit: n entries, or
 *                                        NULL; slacks get 0.
 * MI_LP_ERROR_NULL: NULL h, y, d, status, cols, out, or (mi_lp_row_penalties)
 * NULL distances. Before a solve: MI_LP_ERROR_STATE.
 * MI_LP_ERROR_INVALID_PROBLEM: k < 0, a status outside 0..4, a negative or NaN
 * pivot_tolerance, a distance or unit that is negative, NaN or infinite, a
 * column of cols outside [0, n+m) or not BASIC. On every error nothing is
 * written. k = 0 succeeds and writes nothing. */
typedef struct mi_lp_branch_penalty {
  double down;        /* smallest down candidate, +inf when down_count == 0 */
  double up;
  int32_t down_col;   /* lowest column attaining it, -1 when down_count == 0 */
  int32_t up_col;
  int32_t down_count; /* columns that take part; 0 proves the child infeasible */
  int32_t up_count;
} mi_lp_branch_penalty;
int mi_lp_row_penalties(mi_lp* h, const double* y, int32_t k, const double* d,
                        const int8_t* status, const double* unit, const double* down_dist,
                        const double* up_dist, double pivot_tolerance,
                        mi_lp_branch_penalty* out);
int mi_lp_branching_penalties(mi_lp* h, const int32_t* cols, int32_t k, const double* down_dist,
                              const double* up_dist, const double* unit, double pivot_tolerance,
                              mi_lp_branch_penalty* out, double* left_inverses);

/* The same rows turned on the GPU into Gomory mixed-integer cuts in the space
 * of the structural columns: the GMI formula per column, the slacks eliminated
 * by a second pass over A, and only the kept coefficients of the finished cut
 * (and one 32-byte summary per cut) brought down. Glop's dictionary is
 * [A | I] x = 0; with alpha = rho^T [A | I] for row r of B^-1, row r reads
 * x_B(r) + sum over non-basic j of alpha_j x_j = 0.
 *   mi_lp_row_gomory_cuts   per vector v < k the caller gives f0[v], the
 *                           fractional part of the basic variable in integer
 *                           units, strictly inside (0, 1), and row_unit[v], the
 *                           integer step of the basic column in LP units, finite
 *                           and > 0 (unscaled: 1.0); per column status (n+m,
 *                           MI_LP_BASIC .. MI_LP_FREE) and unit (n+m, 0 for a
 *                           continuous column; NULL: all 0; the meaning is that
 *                           of mi_lp_row_penalties' unit). For every column col
 *                           of [A | I], alpha is bit for bit
 *                           mi_lp_row_combinations' out[v (n+m) + col]. The
 *                           coefficient g, in doubles without FMA:
 *                           1. BASIC and FIXED_VALUE columns: g = +0.0.
 *                           2. A NaN alpha: g = +0.0, counted in bad_count.
 *                           3. Else, unless fabs(alpha) > zero_tolerance
 *                              (strict): g = +0.0.
 *                           4. Else a FREE column: g = +0.0, counted in
 *                              bad_count (a cut with a free non-basic column in
 *                              its support is not valid: the caller drops it).
 *                           5. Else abar = alpha AT_LOWER_BOUND, -alpha
 *                              AT_UPPER_BOUND, and with u = unit[col]:
 *                              u > 0:  t = (abar * u) / row_unit[v];
 *                                      f = t - floor(t);
 *                                      gamma = f <= f0 ? f / f0
 *                                                      : (1.0 - f) / (1.0 - f0);
 *                                      gamma = gamma / u;
 *                              u == 0: t = abar / row_unit[v];
 *                                      gamma = t > 0 ? t / f0
 *                                                    : (-t) / (1.0 - f0).
 *                           6. g = gamma AT_LOWER_BOUND, 0.0 - gamma
 *                              AT_UPPER_BOUND.
 *                           Slack elimination: the slack of row r is
 *                           s_r = -(A x)_r, so with y'[r] = g[n + r] and s = bit
 *                           for bit mi_lp_row_combinations(y')'s value at
 *                           col < n, the cut coefficient is c = g[col] - s, one
 *                           rounded subtraction. Column col is kept iff
 *                           fabs(c) > drop_tolerance (strict, as in the sparse
 *                           rows: +-0.0 is dropped, +-inf kept); a NaN c is
 *                           dropped and counted in bad_count. The cut is
 *                           sum c_j x_j >= rhs over the structural columns. rhs
 *                           is NOT computed (a floating-point sum over the
 *                           columns would fix a summation order): at the node's
 *                           LP point x* every non-basic column sits on its
 *                           bound, so in exact arithmetic
 *                           rhs = 1 + sum_j c_j x*_j, which the caller forms
 *                           from the list it downloads (the Python helper uses
 *                           math.fsum, which does not depend on the order).
 *                           row_starts: k + 1 entries; per vector the kept
 *                           structural columns in strictly increasing order,
 *                           each with c's bits. summaries: one per vector (below;
 *                           an integer sum, exact extrema and lowest indices:
 *                           the same bits in any reduction order). A NULL
 *                           row_starts asks for the summaries alone: no list is
 *                           built, downloaded or stored, and a stored list
 *                           stays. summaries may be NULL; both NULL is
 *                           MI_LP_ERROR_NULL. Everything is the caller's; changes
 *                           no solve state.
 *   mi_lp_gomory_cuts       the same for the k BASIC structural columns cols of
 *                           the current basis: y_j, the side effects and
 *                           left_inverses (k x m, or NULL) are those of
 *                           mi_lp_get_tableau_rows for the rows of cols; status
 *                           = mi_lp_get_state's; unit: n entries, required
 *                           (slacks get 0); row_unit[j] = unit[cols[j]];
 *                           f0[j] = t - floor(t) with t = value / unit[cols[j]],
 *                           value = mi_lp_get_primal[cols[j]].
 *   mi_lp_get_cut_rows      copies the stored lists out (row_starts[k] entries
 *                           each): a sixth store of the handle, apart from the
 *                           others; it lives until the next cut call that builds
 *                           lists, mi_lp_load or mi_lp_destroy.
 * MI_LP_ERROR_NULL: NULL h, y, status, f0, row_unit, cols, unit
 * (mi_lp_gomory_cuts), or row_starts and summaries both NULL. Before a solve:
 * MI_LP_ERROR_STATE; mi_lp_get_cut_rows before any list-building call or after
 * mi_lp_load: MI_LP_ERROR_STATE. MI_LP_ERROR_INVALID_PROBLEM: k < 0, a status
 * outside 0..4, a tolerance that is negative or NaN, an infinite
 * zero_tolerance, a unit that is negative, NaN or infinite, a row_unit that is
 * not finite and > 0, an f0 (given or computed) outside the open interval
 * (0, 1), a column of cols outside [0, n), not BASIC or with unit 0. On every
 * error nothing is written and the store is untouched. k = 0 succeeds, writes
 * row_starts[0] = 0 and stores an empty result.
 * With column shards (MILP_SHARDS) both compute calls return
 * MI_LP_ERROR_STATE ("not with column shards") before any device work: the
 * slack part of g would have to be joined across the shards between the two
 * passes, and that join is not built. */
typedef struct mi_lp_cut_summary {
  double max_abs;    /* largest fabs(c) among the kept entries, 0.0 without one */
  double min_abs;    /* smallest, +inf without one */
  int32_t count;     /* kept entries */
  int32_t bad_count; /* columns of steps 2 and 4 over all n+m columns, plus the NaN c's */
  int32_t max_col;   /* lowest column attaining max_abs, -1 without one */
  int32_t min_col;
} mi_lp_cut_summary;
int mi_lp_row_gomory_cuts(mi_lp* h, const double* y, int32_t k, const int8_t* status,
                          const double* unit, const double* f0, const double* row_unit,
                          double zero_tolerance, double drop_tolerance,
                          int64_t* row_starts, mi_lp_cut_summary* summaries);
int mi_lp_gomory_cuts(mi_lp* h, const int32_t* cols, int32_t k, const double* unit,
                      double zero_tolerance, double drop_tolerance, int64_t* row_starts,
                      mi_lp_cut_summary* summaries, double* left_inverses);
int mi_lp_get_cut_rows(const mi_lp* h, int32_t* cols, double* vals);

/* The other half: the row sums [A | I] x_j of k candidate points in one call
 * that reads A once per panel of up to 16 points (what a caller reads cut
 * violations and row feasibility of roundings, neighbours or ray combinations
 * off, before it pays for mi_lp_batch_solve_bounds). Each sum is Glop's
 * row-activity sum (variable_values.cc:101-131 through
 * ColumnAddMultipleToDenseColumn, sparse.h:389-399):
 *   mi_lp_column_combinations            out[j m + r] starts from +0.0 and takes the
 *                                        entries (col, a) of row r of [A | I] in
 *                                        increasing column order: an entry is skipped when
 *                                        x_j[col] == 0.0 (+0.0 and -0.0; a NaN compares
 *                                        unequal and is not skipped), otherwise
 *                                        acc = acc + x_j[col] * a, every product and every
 *                                        sum rounded separately (no FMA). A row whose live
 *                                        multipliers are all zero gives +0.0. No mask, no
 *                                        sign, no tolerance. Changes no state a later
 *                                        solve reads.
 *   mi_lp_column_combinations_from       the same for the points x_j = base with
 *                                        x_j[cols[i]] = vals[i] for i in
 *                                        [starts[j], starts[j+1]), built on the GPU: only
 *                                        base and the override lists go up. Bit for bit
 *                                        the dense call on the materialised points; an
 *                                        override to +-0.0 skips the entry, NaN and +-inf
 *                                        propagate.
 * x: k x (n+m), vector-major, structural columns then slack columns. base:
 * n+m. out: k x m, vector-major. starts: k+1 entries with starts[0] == 0;
 * cols and vals may be NULL when starts[k] == 0. k = 0 writes nothing and
 * succeeds. MI_LP_ERROR_INVALID_PROBLEM with nothing written: k < 0,
 * starts[0] != 0 or starts decreasing, a column outside [0, n+m), the same
 * column twice within one point. NULL h, x, base, starts or out, or NULL cols
 * or vals with starts[k] > 0: MI_LP_ERROR_NULL. Before a solve:
 * MI_LP_ERROR_STATE. Other errors as mi_lp_row_combinations. */
int mi_lp_column_combinations(mi_lp* h, const double* x, int32_t k, double* out);
int mi_lp_column_combinations_from(mi_lp* h, const double* base, int32_t k,
                                   const int64_t* starts, const int32_t* cols,
                                   const double* vals, double* out);

/* The same activities filtered on the GPU: per point the rows outside their
 * bounds and a 24-byte summary, so that the download is proportional to what
 * is violated and not to k m. With a the value that is bit for bit
 * out[j m + r] of mi_lp_column_combinations on the same point (for the
 * override form: on the materialised points), lo = row_lb[r], hi = row_ub[r]
 * and tol = tolerance, where lo - tol and hi + tol are one rounded double
 * operation each:
 *   violated     row r is violated at point j iff
 *                !(a >= lo - tol) || !(a <= hi + tol). Strict towards
 *                feasibility: an activity exactly on a widened bound is not
 *                violated, one ulp outside it is; a NaN activity is always
 *                violated; +-inf activities follow the comparisons.
 *   amount       of a violated row: +inf when a is NaN, otherwise the larger
 *                of lo - a and a - hi, each rounded once. With the argument
 *                checks below neither difference is NaN for a non-NaN a of a
 *                violated row, and every amount is > 0.
 *   lists        row_starts has k+1 entries, row_starts[k] is the entry
 *                count. Point j's entries are its violated rows in strictly
 *                increasing row order, each with a's bits as its activity.
 *   summaries    one per point: count is the number of violated rows, worst
 *                the largest amount (0.0 when count == 0), worst_row the
 *                lowest row whose amount equals worst (-1 when count == 0),
 *                reserved 0. An integer sum, an exact maximum and a minimum
 *                index: the same bits whatever order the GPU reduces in. A
 *                sum of the amounts is not offered (it would need a fixed
 *                summation order to be reproducible).
 * Two calls, as the sparse rows above:
 *   mi_lp_column_combinations_violations       compute, store the lists in the handle and
 *   mi_lp_column_combinations_from_violations  write row_starts and summaries;
 *   mi_lp_get_violated_rows                    copies the stored rows and activities out,
 *                                              row_starts[k] of each.
 * x, base, starts, cols and vals are those of the dense calls: the points are
 * over all n+m columns of [A | I], so a caller who wants plain A x passes
 * zero slack entries. row_lb / row_ub hold m entries each; either may be NULL
 * and then means the bounds given to mi_lp_load. summaries may be NULL.
 * row_starts may be NULL and means summaries only: no list is built,
 * downloaded or stored, and a previously stored list stays. Both NULL:
 * MI_LP_ERROR_NULL. The stored list is the handle's own, separate from the
 * sparse rows' (mi_lp_get_sparse_rows and the sparse-row calls neither see
 * nor disturb it, nor the other way round); it lives until the next
 * violations call that builds lists, mi_lp_load or mi_lp_destroy.
 * Errors, with nothing written and the stored list untouched:
 * MI_LP_ERROR_INVALID_PROBLEM for k < 0, a tolerance that is negative, NaN
 * or infinite, a NaN bound, row_lb[r] == +inf or row_ub[r] == -inf (lb > ub
 * is allowed: such a row is violated at every point), and, for the override
 * form, every condition of mi_lp_column_combinations_from. MI_LP_ERROR_NULL:
 * NULL pointers as in the dense calls. MI_LP_ERROR_STATE: before a solve;
 * mi_lp_get_violated_rows before any list-building call, or after
 * mi_lp_load. k = 0 succeeds, writes row_starts[0] = 0 if row_starts is
 * given and stores an empty list. Changes no state a later solve reads. */
typedef struct mi_lp_point_violations {
  int64_t count;
  double worst;
  int32_t worst_row;
  int32_t reserved;
} mi_lp_point_violations;
int mi_lp_column_combinations_violations(mi_lp* h, const double* x, int32_t k,
                                         const double* row_lb, const double* row_ub,
                                         double tolerance, int64_t* row_starts,
                                         mi_lp_point_violations* summaries);
int mi_lp_column_combinations_from_violations(mi_lp* h, const double* base, int32_t k,
                                              const int64_t* starts, const int32_t* cols,
                                              const double* vals, const double* row_lb,
                                              const double* row_ub, double tolerance,
                                              int64_t* row_starts,
                                              mi_lp_point_violations* summaries);
int mi_lp_get_violated_rows(const mi_lp* h, int32_t* rows, double* activities);

/* Bound sets instead of points: the activity range of every row of A under
 * each of k bound sets (the children of a node, as mi_lp_batch_solve_bounds
 * takes them), in one call that reads A once per panel of up to 16 sets: what
 * a caller reads a child's infeasibility or its residual activities off before
 * it pays for a solve. Bound sets are over the n structural columns only:
 * lbs / ubs are k x n, row-major, as for mi_lp_batch_solve_bounds, and the
 * slack entry that closes every row of [A | I] (column >= n) is no part of a
 * range. For row r and set j, with l = lbs[j], u = ubs[j]:
 *   lo = +0.0; hi = +0.0; lo_inf = 0; hi_inf = 0
 *   for the entries (col, a) of row r with col < n, in increasing column order:
 *     if a == 0.0: continue                       (+0.0 and -0.0)
 *     (bl, bh) = (l[col], u[col]) if a > 0.0 else (u[col], l[col])
 *     if isinf(bl): lo_inf += 1  else: lo = lo + a * bl
 *     if isinf(bh): hi_inf += 1  else: hi = hi + a * bh
 * every product and every sum rounded separately (no FMA). An infinite bound
 * of EITHER sign on the side it is read from is counted and not added: l =
 * +inf makes the row's minimum unknown (lo_inf > 0), never +inf. A NaN bound
 * is not infinite and propagates into the sum; a NaN coefficient takes the
 * else branch; nothing examines l > u. A row without structural entries gives
 * (+0.0, +0.0, 0, 0).
 *   mi_lp_bound_activity_ranges       min_activity[j m + r] = lo,
 *                                     max_activity[j m + r] = hi (k x m each,
 *                                     vector-major), inf_counts[(j m + r) 2 ..]
 *                                     = (lo_inf, hi_inf), k x m x 2 int32; it
 *                                     may be NULL. The caller folds: the
 *                                     minimum is -inf when lo_inf > 0.
 *   mi_lp_bound_activity_ranges_from  the same for the sets l_j = base_lb with
 *                                     l_j[cols[i]] = new_lbs[i], u_j = base_ub
 *                                     with u_j[cols[i]] = new_ubs[i] for i in
 *                                     [starts[j], starts[j+1]), built on the
 *                                     GPU. Bit for bit the dense form on the
 *                                     materialised sets.
 * Screening, with lb = row_lb[r], ub = row_ub[r], tol = tolerance:
 *   g = -inf
 *   if lo_inf == 0: d = lo - ub;  if d > g: g = d
 *   if hi_inf == 0: d = lb - hi;  if d > g: g = d
 *   row r proves set j infeasible iff g > tol
 * each difference rounded once. A NaN d never replaces g, so g is never NaN:
 * a NaN bound or a sum that overflowed can only make the screen say "not
 * proven". The screen is conservative by construction: it never reports a
 * set that has a point within the bounds and the rows.
 *   lists      row_starts has k+1 entries; set j's entries are its proving
 *              rows in strictly increasing order, each with g's bits as its
 *              amount.
 *   summaries  mi_lp_point_violations: count the number of proving rows, worst
 *              the largest g (0.0 when count == 0), worst_row the lowest row
 *              attaining it (-1 when count == 0). An integer sum, an exact
 *              maximum and a minimum index: the same bits whatever order the
 *              GPU reduces in.
 *   mi_lp_bound_infeasible_rows       compute, store the lists in the handle and
 *   mi_lp_bound_infeasible_rows_from  write row_starts and summaries;
 *   mi_lp_get_infeasible_rows         copies the stored rows and amounts out,
 *                                     row_starts[k] of each.
 * row_lb / row_ub hold m entries each; either may be NULL and then means the
 * bounds given to mi_lp_load; +-inf on either side is allowed. summaries may
 * be NULL. row_starts may be NULL and means summaries only: no list is built,
 * downloaded or stored, and a previously stored list stays. Both NULL:
 * MI_LP_ERROR_NULL. The stored list is a third store of the handle, separate
 * from the sparse rows' and from the violated rows' (none sees or disturbs
 * another); it lives until the next call that builds these lists, mi_lp_load
 * or mi_lp_destroy.
 * Errors, with nothing written and the stored list untouched:
 * MI_LP_ERROR_INVALID_PROBLEM for k < 0, a tolerance that is negative, NaN or
 * infinite, a NaN row bound, starts[0] != 0 or starts decreasing, a column
 * outside [0, n), the same column twice within one set. MI_LP_ERROR_NULL:
 * NULL h, lbs, ubs, base_lb, base_ub, starts, min_activity or max_activity,
 * or NULL cols, new_lbs or new_ubs with starts[k] > 0. MI_LP_ERROR_STATE:
 * before a solve; mi_lp_get_infeasible_rows before any list-building call, or
 * after mi_lp_load. k = 0 succeeds: the range calls write nothing, the
 * screening writes row_starts[0] = 0 if row_starts is given and stores an
 * empty list. No solve uses these calls and they change no state a later
 * solve reads. */
int mi_lp_bound_activity_ranges(mi_lp* h, const double* lbs, const double* ubs, int32_t k,
                                double* min_activity, double* max_activity,
                                int32_t* inf_counts);
int mi_lp_bound_activity_ranges_from(mi_lp* h, const double* base_lb, const double* base_ub,
                                     int32_t k, const int64_t* starts, const int32_t* cols,
                                     const double* new_lbs, const double* new_ubs,
                                     double* min_activity, double* max_activity,
                                     int32_t* inf_counts);
int mi_lp_bound_infeasible_rows(mi_lp* h, const double* lbs, const double* ubs, int32_t k,
                                const double* row_lb, const double* row_ub, double tolerance,
                                int64_t* row_starts, mi_lp_point_violations* summaries);
int mi_lp_bound_infeasible_rows_from(mi_lp* h, const double* base_lb, const double* base_ub,
                                     int32_t k, const int64_t* starts, const int32_t* cols,
                                     const double* new_lbs, const double* new_ubs,
                                     const double* row_lb, const double* row_ub,
                                     double tolerance, int64_t* row_starts,
                                     mi_lp_point_violations* summaries);
int mi_lp_get_infeasible_rows(const mi_lp* h, int32_t* rows, double* amounts);

/* One round of bound propagation over those ranges: from each row's activity
 * range and bounds, the implied bounds of every structural column it holds,
 * per bound set, in the same call (the ranges never leave the GPU). Per set j,
 * with l = lbs[j] and u = ubs[j], let (lo, hi, lo_inf, hi_inf)[r] be row r's
 * result of mi_lp_bound_activity_ranges, bit for bit, and rlb = row_lb, rub =
 * row_ub. For every column c < n:
 *   nl = l[c]; nu = u[c]
 *   for the entries (r, a) of column c, in any order:
 *     if a == 0.0 or a is NaN: continue
 *     up = a > 0.0
 *     (bl, bh) = (l[c], u[c]) if up else (u[c], l[c])    what c fed into lo / hi
 *     for (rb, s, cnt, b, tightens_upper) in ((rub[r], lo[r], lo_inf[r], bl, up),
 *                                             (rlb[r], hi[r], hi_inf[r], bh, !up)):
 *       if !isfinite(rb): continue
 *       if   cnt == 0:              res = s - a * b      product and difference
 *                                                        rounded separately
 *       elif cnt == 1 and isinf(b): res = s              c is the one infinite term
 *       else: continue
 *       q = (rb - res) / a                               one difference, one division
 *       if !isfinite(q): continue                        NaN and overflow: no candidate
 *       q = q + 0.0                                      -0.0 becomes +0.0
 *       if tightens_upper: if q < nu: nu = q
 *       else:              if q > nl: nl = q
 * No FMA anywhere. A NaN own bound stays NaN (every comparison with it fails);
 * otherwise nl >= l and nu <= u. A column without entries keeps its bounds.
 * Every result is a max or a min of independently rounded candidates, and the
 * q + 0.0 step gives equal candidates equal bits, so the result does not
 * depend on the order of the entries or of the GPU's reduction. The rule is
 * the textbook one in doubles and is NOT outward-rounded: an implied bound can
 * be off by the rounding of its sum in either direction, and a caller that
 * needs a safe bound widens it itself. The tolerance below is a filter, not a
 * safety margin.
 *   mi_lp_bound_implied_bounds       new_lbs[j n + c] = nl, new_ubs[j n + c] =
 *                                    nu, k x n each, set-major.
 *   mi_lp_bound_implied_bounds_from  the same for the sets base + overrides of
 *                                    mi_lp_bound_activity_ranges_from (ov_lbs /
 *                                    ov_ubs are its new_lbs / new_ubs). Bit for
 *                                    bit the dense form on the materialised sets.
 * The filtered form keeps, per set, with tol = tolerance:
 *   moved    = (nl - l[c] > tol) || (u[c] - nu > tol)    inf - inf is NaN: no
 *   cross    = nl - nu;  crossing = cross > tol
 *   changed  = l[c] or u[c] differs IN BITS from base_lb[c] / base_ub[c]
 *   dense form: keep iff moved || crossing;  override form: keep iff moved ||
 *   crossing || changed
 * so a column whose own bounds already cross is kept without any move, and in
 * the override form a set's list is its complete override list relative to
 * the base: fed back unchanged as overrides it gives a second round,
 * mi_lp_bound_infeasible_rows_from, or the child for mi_lp_batch_solve_bounds.
 *   lists      col_starts has k+1 entries; set j's entries are its kept
 *              columns in strictly increasing order, each with nl and nu.
 *   summaries  mi_lp_point_violations: count the number of kept columns, worst
 *              the largest cross among the crossing columns (0.0 without one),
 *              worst_row the lowest COLUMN attaining it (-1 without one; count
 *              > 0 with worst_row == -1 is the ordinary case). A set is proven
 *              infeasible by propagation iff worst_row >= 0.
 *   mi_lp_bound_tightened_columns       compute, store the lists in the handle
 *   mi_lp_bound_tightened_columns_from  and write col_starts and summaries;
 *   mi_lp_get_tightened_columns         copies the stored columns and bounds
 *                                       out, col_starts[k] of each.
 * NULL handling, k = 0, the state before a solve and every error code are
 * those of mi_lp_bound_infeasible_rows(_from): row_lb / row_ub may be NULL
 * (the loaded bounds), +-inf allowed, a NaN row bound is
 * MI_LP_ERROR_INVALID_PROBLEM, as are a bad tolerance, bad starts and a
 * repeated column; col_starts == NULL means summaries only, and a previously
 * stored list stays. The stored lists are a fourth store of the handle; it
 * neither sees nor disturbs the other three. With MILP_SHARDS the calls stay
 * on the unsplit handle. No solve uses these calls and they change no state a
 * later solve reads.
 * Integer rounding of the results and more than one round per call are
 * mi_lp_bound_propagate's (below), not these calls'.
 * Out of scope: a packed or double2 layout of the three range blocks; a
 * per-column choice between the two kernel shapes. */
int mi_lp_bound_implied_bounds(mi_lp* h, const double* lbs, const double* ubs, int32_t k,
                               const double* row_lb, const double* row_ub, double* new_lbs,
                               double* new_ubs);
int mi_lp_bound_implied_bounds_from(mi_lp* h, const double* base_lb, const double* base_ub,
                                    int32_t k, const int64_t* starts, const int32_t* cols,
                                    const double* ov_lbs, const double* ov_ubs,
                                    const double* row_lb, const double* row_ub, double* new_lbs,
                                    double* new_ubs);
int mi_lp_bound_tightened_columns(mi_lp* h, const double* lbs, const double* ubs, int32_t k,
                                  const double* row_lb, const double* row_ub, double tolerance,
                                  int64_t* col_starts, mi_lp_point_violations* summaries);
int mi_lp_bound_tightened_columns_from(mi_lp* h, const double* base_lb, const double* base_ub,
                                       int32_t k, const int64_t* starts, const int32_t* cols,
                                       const double* ov_lbs, const double* ov_ubs,
                                       const double* row_lb, const double* row_ub,
                                       double tolerance, int64_t* col_starts,
                                       mi_lp_point_violations* summaries);
int mi_lp_get_tightened_columns(const mi_lp* h, int32_t* cols, double* new_lbs, double* new_ubs);

/* Node propagation: those rounds repeated on the GPU until nothing moves, a
 * column crosses or max_rounds is reached, with integer columns rounded; the
 * bound sets, the ranges and the implied bounds stay on the GPU between
 * rounds and 24 bytes per set come down per round. Inputs beside the sets:
 * row_lb / row_ub as above; is_integer, n bytes, non-zero marks an integer
 * column, NULL means none; tolerance >= 0, finite; integrality_tolerance in
 * [0, 0.5), finite; max_rounds >= 1. Per set j, with own bounds (l, u):
 *   status = MI_LP_PROPAGATE_ROUND_LIMIT; rounds = 0; moves = 0
 *   worst = 0.0; worst_col = -1
 *   for round = 1 .. max_rounds:
 *     (nl, nu) = the result of mi_lp_bound_implied_bounds on (l, u), bit for bit
 *     for every column c < n:
 *       if is_integer[c]: nl[c] = ceil(nl[c] - integrality_tolerance) + 0.0
 *                         nu[c] = floor(nu[c] + integrality_tolerance) + 0.0
 *       moved = (nl[c] - l[c] > tolerance) || (u[c] - nu[c] > tolerance)
 *       if moved: (l'[c], u'[c]) = (nl[c], nu[c])      BOTH sides
 *       else:     (l'[c], u'[c]) = (l[c], u[c])
 *       cross = l'[c] - u'[c];  crossing = cross > tolerance
 *     (l, u) = (l', u'); rounds = round; moves += number of moved columns
 *     if some column crosses: status = MI_LP_PROPAGATE_INFEASIBLE
 *                             worst = the largest cross
 *                             worst_col = the lowest column attaining it; stop
 *     if no column moved:     status = MI_LP_PROPAGATE_FIXPOINT; stop
 * The difference and the sum inside ceil / floor are one rounded operation
 * each, ceil and floor are exact and + 0.0 turns -0.0 into +0.0; an infinity
 * stays and a NaN stays. inf - inf and every difference with a NaN are NaN
 * and fail their comparison: a NaN own bound stays NaN and never moves. A set
 * whose own bounds already cross stops INFEASIBLE in round 1, and an
 * INFEASIBLE set keeps the bounds of the round that found the crossing. A
 * moved column takes both new bounds, as a kept column of
 * mi_lp_bound_tightened_columns_from does when its list is fed back; rounding
 * can therefore put the side that did not move below (above) the own bound by
 * less than one. The rounds are Jacobi rounds: every column of a round reads
 * the bounds of the round's start, so with the one-round rule's order
 * independence every bit of the result is independent of the reduction
 * order, the kernel shape, the panel width and of which other sets share the
 * call. Like the one-round rule it is NOT outward-rounded: the tolerances are
 * filters, not safety margins.
 * moves is exact: it counts moved columns only. A column that crosses without
 * having moved exists only in round 1 (its own bounds cross); it is kept out
 * of moves by a second count over move-only keys, made for the sets that stop
 * INFEASIBLE in round 1 and for no other.
 * With is_integer == NULL and tolerance == 0, a set that is not INFEASIBLE
 * before round R has after R rounds exactly the bits of R calls of
 * mi_lp_bound_tightened_columns_from, each list fed back as that set's
 * overrides. (With a tolerance > 0 the fed-back list also carries nl and nu of
 * the columns it keeps only because they differ from the base, which this
 * rule leaves at their own bounds while they move by no more than the
 * tolerance.)
 *   mi_lp_bound_propagate       dense sets in; the final (l, u) into new_lbs /
 *                               new_ubs, k x n each, set-major, and one
 *                               mi_lp_propagation per set (summaries may be
 *                               NULL). kept = the number of columns whose
 *                               final l or u differs in bits from the input.
 *   mi_lp_bound_propagate_from  the same for the sets base + overrides, built
 *                               on the GPU; bit for bit the dense form on the
 *                               materialised sets, kept included.
 *   mi_lp_bound_propagated_columns_from
 *                               keeps per set the columns whose final l or u
 *                               differs IN BITS from base_lb / base_ub, or
 *                               that cross (l - u > tolerance), ascending,
 *                               each with its final l and u; kept = the
 *                               length of the set's list. The list is the
 *                               set's complete override list relative to the
 *                               base: it feeds mi_lp_bound_infeasible_rows_from,
 *                               another propagate call or (materialised)
 *                               mi_lp_batch_solve_bounds. Stores the lists and
 *                               writes col_starts (k + 1) and summaries;
 *                               col_starts == NULL means summaries only, and a
 *                               previously stored list stays.
 *   mi_lp_get_propagated_columns  copies the stored columns and bounds out,
 *                               col_starts[k] of each.
 * NULL handling, k = 0, the state before a solve, MILP_SHARDS (the calls stay
 * on the unsplit handle) and every error code are those of
 * mi_lp_bound_tightened_columns(_from); in addition max_rounds < 1 and an
 * integrality_tolerance that is negative, NaN or >= 0.5 are
 * MI_LP_ERROR_INVALID_PROBLEM. Nothing is written on an error. The stored
 * lists are a fifth store of the handle; it neither sees nor disturbs the
 * other four. No solve uses these calls and they change no state a later
 * solve reads.
 * Out of scope: fusing the apply step into the implied-bound kernels; a
 * device-side round loop without the per-round 24 k byte download; a row-side
 * infeasibility screen per round (a caller runs
 * mi_lp_bound_infeasible_rows_from on the result); outward rounding; a
 * per-column choice between the two implied-bound kernel shapes; lists in the
 * dense-input form; using the result inside any solve. */
#define MI_LP_PROPAGATE_ROUND_LIMIT 0
#define MI_LP_PROPAGATE_FIXPOINT 1
#define MI_LP_PROPAGATE_INFEASIBLE 2
typedef struct mi_lp_propagation {
  int32_t status;    /* MI_LP_PROPAGATE_* */
  int32_t rounds;    /* rounds this set took part in */
  int64_t moves;     /* moved columns, summed over the rounds */
  double worst;      /* INFEASIBLE: the largest cross; else 0.0 */
  int32_t worst_col; /* INFEASIBLE: the lowest column attaining it; else -1 */
  int32_t kept;      /* see the calls above */
} mi_lp_propagation;
int mi_lp_bound_propagate(mi_lp* h, const double* lbs, const double* ubs, int32_t k,
                          const uint8_t* is_integer, const double* row_lb, const double* row_ub,
                          double tolerance, double integrality_tolerance, int32_t max_rounds,
                          double* new_lbs, double* new_ubs, mi_lp_propagation* summaries);
int mi_lp_bound_propagate_from(mi_lp* h, const double* base_lb, const double* base_ub, int32_t k,
                               const int64_t* starts, const int32_t* cols, const double* ov_lbs,
                               const double* ov_ubs, const uint8_t* is_integer,
                               const double* row_lb, const double* row_ub, double tolerance,
                               double integrality_tolerance, int32_t max_rounds, double* new_lbs,
                               double* new_ubs, mi_lp_propagation* summaries);
int mi_lp_bound_propagated_columns_from(mi_lp* h, const double* base_lb, const double* base_ub,
                                        int32_t k, const int64_t* starts, const int32_t* cols,
                                        const double* ov_lbs, const double* ov_ubs,
                                        const uint8_t* is_integer, const double* row_lb,
                                        const double* row_ub, double tolerance,
                                        double integrality_tolerance, int32_t max_rounds,
                                        int64_t* col_starts, mi_lp_propagation* summaries);
int mi_lp_get_propagated_columns(const mi_lp* h, int32_t* cols, double* new_lbs, double* new_ubs);

/* interrupt may be NULL; a non-zero value stops the solve like a time limit
 * (glop_interface.cc:138-140). */
int mi_lp_solve(mi_lp* h, const volatile int32_t* interrupt, mi_lp_result* out);

int mi_lp_get_primal(const mi_lp* h, double* x);            /* n */
int mi_lp_get_reduced_costs(const mi_lp* h, double* rc);    /* n */
int mi_lp_get_duals(const mi_lp* h, double* y);             /* m */
int mi_lp_get_activities(const mi_lp* h, double* act);      /* m */
int mi_lp_get_statuses(const mi_lp* h, int8_t* var, int8_t* cons); /* n, m */
int mi_lp_get_basis(const mi_lp* h, int32_t* basis);        /* m, column ids */
int mi_lp_get_state(const mi_lp* h, int8_t* statuses);      /* n+m */
int mi_lp_get_primal_ray(const mi_lp* h, double* ray);      /* n+m */
int mi_lp_get_dual_ray(const mi_lp* h, double* ray);        /* m */
int mi_lp_get_dual_ray_row_combination(const mi_lp* h, double* v); /* n+m */

/* Benchmark slicing: mi_lp_begin starts Solve() on a worker thread that
 * parks when num_iterations reaches pause_at (negative = never).
 * mi_lp_run_until moves the pause point and blocks until the worker parks
 * again or finishes (*finished = 1); the device stream is synchronized
 * before it returns. mi_lp_finish joins and fills the result. */
int mi_lp_begin(mi_lp* h, int64_t pause_at);
int mi_lp_run_until(mi_lp* h, int64_t pause_at, int32_t* finished,
                    int64_t* iterations);
int mi_lp_finish(mi_lp* h, mi_lp_result* out);
/* Interrupts a begun solve at its next time-limit check (the interrupt flag
 * of glop_interface.cc:186-189); follow with mi_lp_finish. */
int mi_lp_stop(mi_lp* h);

int mi_lp_get_kernel_stats(const mi_lp* h, mi_lp_kernel_stats* s);
int mi_lp_reset_kernel_stats(mi_lp* h);
/* enable != 0: bracket every hot kernel with HIP events. The events are
 * read back when the stats are collected (or every 512 launches): timing adds
 * no synchronization to the iteration it measures. */
int mi_lp_set_kernel_timing(mi_lp* h, int32_t enable);
/* The same for the kernel ids whose bits are set in id_mask (bit k = id k of
 * mi_lp_kernel_stats; 0 = off): a benchmark times its dominant kernel
 * without paying two event records on every other launch. */
int mi_lp_set_kernel_timing_ids(mi_lp* h, uint32_t id_mask);

/* Window statistics for the benchmark harness (the reference keeps the same
 * numbers in RevisedSimplex's stats, revised_simplex.h:717-760, and
 * BasisFactorization's, basis_representation.h:359-373).
 * mi_lp_record_iteration_times: enable a timestamp (seconds since Solve()
 * started) per completed iteration; call before mi_lp_begin or while paused.
 * mi_lp_get_iteration_times copies min(cap, count) of them and returns count
 * (a negative error code when the solve is running). */
typedef struct mi_lp_run_counters {
  int64_t factorizations;       /* LU factorizations computed so far */
  double factorization_seconds; /* host wall time spent in them */
  int64_t iterations;           /* RevisedSimplex::GetNumberOfIterations */
  /* The device schedule of the current factorization's U (FTRAN's dense U
   * solve, 0 when none was built): dependency levels, computed outputs,
   * gather entries. A level is a dependency hop of the solve. */
  int64_t u_levels;
  int64_t u_outputs;
  int64_t u_entries;
  /* Device dual simplex segments (MILP_SDUAL; phase-II dual iterations run
   * whole on one workgroup) and the iterations they ran, since creation. */
  int64_t sdual_segments;
  int64_t sdual_iterations;
} mi_lp_run_counters;
int mi_lp_record_iteration_times(mi_lp* h, int32_t enable);
int64_t mi_lp_get_iteration_times(const mi_lp* h, double* out, int64_t cap);
int mi_lp_get_run_counters(const mi_lp* h, mi_lp_run_counters* c);

/* Cross-process split of ONE LP over `world` processes (the
 * reference's sharding pattern is pdlp/sharder.h:34-160): every process loads
 * the same LP into its handle and runs the same host control flow; process
 * `rank` keeps column block `rank` of [A | I] (64-aligned blocks balanced by
 * entries, as MILP_SHARDS cuts them) on its own GPU. Each per-column device
 * operation runs on the owned block, and its results are joined in block
 * order through `allgather`: the update row's list, the pricing reduced
 * costs, the dual ratio test's filtered breakpoints (the all-reduce(min) of
 * the bound is implicit: each block filters under its own bound, a superset
 * of the joint filter) and the entering column's coefficient. Results are
 * bit-identical to the unsplit engine. allgather(ctx, send, send_bytes, recv,
 * recv_bytes) must place every rank's bytes in rank order (recv_bytes[r]
 * bytes from rank r, all ranks' sizes known to the caller) and return 0.
 * Call before mi_lp_load; world <= 1 or allgather == NULL turns it off. */
typedef int (*mi_lp_allgather_fn)(void* ctx, const void* send, int64_t send_bytes, void* recv,
                                  const int64_t* recv_bytes);
int mi_lp_set_exchange(mi_lp* h, int32_t rank, int32_t world, void* ctx,
                       mi_lp_allgather_fn allgather);

/* Same-node exchange for mi_lp_set_exchange (engine/exchange.cc): an
 * all-gather of host bytes through one POSIX shared-memory segment, so the
 * split's per-iteration joins run in C++ with no Python and no socket on the
 * path (the joined messages are consumed by every rank's host control flow).
 * Rank 0 creates `name` (a fresh shm name, e.g. "/mi_lp_<uuid>", distributed
 * by the caller), the others attach; the name is unlinked once all `world`
 * ranks attached. Messages longer than slot_bytes go in several rounds.
 * Pass (ctx = the exchange, allgather = mi_exchange_allgather) to
 * mi_lp_set_exchange; close after the handle is done with it. */
typedef struct mi_exchange mi_exchange;
int mi_exchange_open(const char* name, int32_t rank, int32_t world, int64_t slot_bytes,
                     mi_exchange** out);
int mi_exchange_allgather(void* ctx, const void* send, int64_t send_bytes, void* recv,
                          const int64_t* recv_bytes);
void mi_exchange_close(mi_exchange* x);

/* Batch API: solves count independent LPs already loaded in handles (all on
 * the same device) on num_threads host threads; each thread drives several
 * LPs as fibers (MILP_BATCH_FIBERS, default 4) switching at device waits, and
 * their one-launch update rows go out in batched launches (one workgroup per
 * LP request; MILP_SMALL_BATCH=0 turns that off). Results are per LP and
 * identical to one-at-a-time solves.
 * Returns non-OK only for bad arguments; each LP's outcome (including its
 * error code) is in results[i]. No exception crosses this boundary. */
int mi_lp_batch_solve(mi_lp* const* handles, int32_t count, int32_t num_threads,
                      mi_lp_result* results);
/* mi_lp_batch_solve over several GPUs of one process (SURVEY 8(b)
 * mi_lp_batch_solve(hs, count, num_gpus, ...)): every handle's device must be
 * in [0, num_gpus); each device's handles run on a pool of threads_per_gpu
 * threads of their own, all devices at once. */
int mi_lp_batch_solve_gpus(mi_lp* const* handles, int32_t count, int32_t num_gpus,
                           int32_t threads_per_gpu, mi_lp_result* results);
/* Batched children of one search node: count LPs that share
 * the workers' loaded matrix and differ in variable bounds (lbs/ubs are
 * count x n, row-major), each warm-started from warm_state (n+m statuses,
 * may be NULL, else warm_len must be n+m) like LoadStateForNextSolve. The
 * workers may be on several GPUs; they run on at most 16 host threads
 * (MILP_BATCH_THREADS), dealt device by device, a thread's workers as fibers
 * with batched small-LP launches (as mi_lp_batch_solve), every worker pulling
 * the next child from one shared counter. A child whose bounds or state cannot be loaded is
 * not solved: results[i] = {ABNORMAL, that error code}. */
int mi_lp_batch_solve_bounds(mi_lp* const* workers, int32_t num_workers, int32_t count,
                             const double* lbs, const double* ubs, const int8_t* warm_state,
                             int32_t warm_len, mi_lp_result* results);

/* Multi-GPU bound sharing over RCCL: the batched LPs are
 * sharded across GPUs with no data-path collective; the one exchange is the
 * search's objective bound, an all-reduce(min) of one float64 over xGMI —
 * the cross-GPU analogue of SharedResponseManager::UpdateInnerObjectiveBounds
 * (ortools/sat/synchronization.h:306), which a CP-SAT worker thread calls
 * with its LP's bound. One communicator per rank (process or thread), bound
 * to a GPU; its unique id is created once (mi_lp_comm_get_unique_id, rank 0)
 * and handed to every rank out of band, as ncclGetUniqueId's. RCCL is ROCm's
 * librccl.so.1, opened privately (dlopen RTLD_LOCAL). Errors: MI_LP_ERROR_DEVICE
 * (message in mi_lp_comm_last_error; with c == NULL, why RCCL is unusable). */
typedef struct mi_lp_comm mi_lp_comm;
enum { MI_LP_COMM_ID_BYTES = 128 };
enum { MI_LP_BOUND_MIN = 0, MI_LP_BOUND_MAX = 1 };
int mi_lp_comm_get_unique_id(uint8_t* id /* MI_LP_COMM_ID_BYTES */);
/* Collective over the nranks ranks (ncclCommInitRank): blocks until all join. */
int mi_lp_comm_create(const uint8_t* id, int32_t nranks, int32_t rank, int32_t device,
                      mi_lp_comm** out);
int32_t mi_lp_comm_rank(const mi_lp_comm* c);
int32_t mi_lp_comm_size(const mi_lp_comm* c);
/* *bound <- min (MI_LP_BOUND_MIN) or max over the ranks of *bound: the value
 * goes through an 8-byte device buffer and one ncclAllReduce(ncclFloat64);
 * returns once the result is on the host. Every rank must call it. */
int mi_lp_share_bound(mi_lp_comm* c, double* bound, int32_t op);
/* The same reduction in place on a caller's device buffer of count doubles,
 * and an all-gather of bytes_per_rank bytes per rank between device buffers
 * (recv holds nranks blocks in rank order). Synchronous. */
int mi_lp_comm_allreduce_device(mi_lp_comm* c, double* d_values, int64_t count, int32_t op);
int mi_lp_comm_allgather_device(mi_lp_comm* c, const void* d_send, void* d_recv,
                                int64_t bytes_per_rank);
const char* mi_lp_comm_last_error(const mi_lp_comm* c);
void mi_lp_comm_destroy(mi_lp_comm* c);

/* MPS ingestion: the reader that fills the
 * LinearProgram handed to mi_lp_load, replacing
 *   glop::MPSReader::ParseFile / ParseString   (ortools/lp_data/mps_reader.h:39-60,
 *                                               mps_reader_template.h ParseFile)
 * with the LinearProgram data wrapper (mps_reader.cc:22-112). Formats as
 * MPSReaderFormat: auto-detection tries fixed, then free. On error the return
 * code is MI_LP_ERROR_INVALID_PROBLEM (absl::InvalidArgumentError upstream)
 * and mi_mps_error() holds the message; the model is always allocated and
 * must be released with mi_mps_free. The matrix comes back cleaned up (CSC,
 * rows sorted per column, no zeros), ready for mi_lp_load. */
typedef struct mi_mps_model mi_mps_model;
enum { MI_MPS_AUTO = 0, MI_MPS_FREE = 1, MI_MPS_FIXED = 2 };
int mi_mps_read_file(const char* path, int32_t format, mi_mps_model** out,
                     int32_t* format_used);
int mi_mps_parse_string(const char* text, int32_t format, mi_mps_model** out,
                        int32_t* format_used);
const char* mi_mps_error(const mi_mps_model* m);
int mi_mps_dims(const mi_mps_model* m, int32_t* num_rows, int32_t* num_cols, int64_t* nnz);
/* Any output pointer may be NULL. col_starts has num_cols + 1 entries. */
int mi_mps_get(const mi_mps_model* m, int64_t* col_starts, int32_t* row_idx, double* vals,
               double* col_lb, double* col_ub, double* row_lb, double* row_ub, double* obj,
               double* obj_offset, int32_t* maximize, int8_t* is_integer);
const char* mi_mps_name(const mi_mps_model* m);
const char* mi_mps_col_name(const mi_mps_model* m, int32_t col);
const char* mi_mps_row_name(const mi_mps_model* m, int32_t row);
void mi_mps_free(mi_mps_model* m);

/* LPSolver layer: what glop::LPSolver::SolveWithTimeLimit
 * (ortools/glop/lp_solver.cc:150-262) does around RevisedSimplex::Solve for
 * the MPSolver path (glop_interface.cc:104-169): IsCleanedUp / IsValid checks,
 * ScalingPreprocessor::Run (preprocessor.cc:3855-3876: SparseMatrixScaler
 * geometric + equilibration passes, matrix_scaler.cc; ScaleObjective /
 * ScaleBounds, lp_data.cc:1190-1258), the engine solve on handle h, then
 * ScalingPreprocessor::RecoverSolution (preprocessor.cc:3878-3912) and the
 * value part of LoadAndVerifySolution (lp_solver.cc:334-367: reduced costs,
 * Kahan objective, strong-optimal moves, activities). With use_preprocessing
 * (the default, as in Glop) MainLpPreprocessor's passes run before the
 * scaling and their postsolve after it (engine/presolve.cc),
 * and the postsolved solution goes through IsProblemSolutionConsistent
 * (lp_solver.cc:679-790; inconsistent = ABNORMAL). out->objective is the
 * unscaled problem objective; the arrays (n / m entries, any may be NULL)
 * are the unscaled solution. An invalid LP gives MI_LP_OK with
 * problem_status MI_LP_INVALID_PROBLEM, as LPSolver returns it. */
enum { MI_LP_SCALING_DEFAULT = 0, MI_LP_EQUILIBRATION = 1, MI_LP_LINEAR_PROGRAM = 2 };
enum { MI_LP_NO_COST_SCALING = 0, MI_LP_CONTAIN_ONE_COST_SCALING = 1,
       MI_LP_MEAN_COST_SCALING = 2, MI_LP_MEDIAN_COST_SCALING = 3 };
typedef struct mi_lp_solver_params {
  int32_t use_scaling;                      /* 16, true */
  int32_t scaling_method;                   /* 57, EQUILIBRATION (LINEAR_PROGRAM not built:
                                               geometric + equilibration, as upstream
                                               when its scaling LP fails) */
  int32_t cost_scaling;                     /* 60, CONTAIN_ONE_COST_SCALING */
  int32_t provide_strong_optimal_guarantee; /* 24, true */
  double max_valid_magnitude;               /* 199, 1e30 */
  /* Presolve: MainLpPreprocessor's passes (preprocessor.cc:76-147), on by
   * default as in Glop (parameters.proto:326); 0 = scaling only. DESIGN.md §6a. */
  int32_t use_preprocessing;                /* 34, true */
  int32_t use_implied_free_preprocessor;    /* 67, true */
  int32_t solve_dual_problem;               /* 20, LET_SOLVER_DECIDE (ALWAYS_DO 0,
                                               NEVER_DO 1, LET_SOLVER_DECIDE 2) */
  int32_t change_status_to_imprecise;       /* 58, true: LoadAndVerifySolution may
                                               report IMPRECISE */
  double dualizer_threshold;                /* 21, 1.5 */
  double preprocessor_zero_tolerance;       /* 39, 1e-9 */
  double solution_feasibility_tolerance;    /* 22, 1e-6 */
  double drop_tolerance;                    /* 52, 1e-14 */
} mi_lp_solver_params;
void mi_lp_solver_params_default(mi_lp_solver_params* p);
/* ScalingPreprocessor::Run alone, in place on the caller's arrays (no device
 * needed): row_scale (m) / col_scale (n) receive SparseMatrixScaler's
 * unscaling factors, *cost_factor / *bound_factor the divisors of
 * ScaleObjective / ScaleBounds. With use_scaling = 0 nothing changes and
 * every factor is 1. */
int mi_lp_scale(const mi_lp_solver_params* sp, int32_t m, int32_t n, const int64_t* col_starts,
                const int32_t* row_idx, double* vals, double* col_lb, double* col_ub,
                double* row_lb, double* row_ub, double* obj, double* obj_offset,
                double* obj_scale, double* row_scale, double* col_scale, double* cost_factor,
                double* bound_factor);
int mi_lp_solver_solve(mi_lp* h, const mi_lp_solver_params* sp, int32_t m, int32_t n,
                       const int64_t* col_starts, const int32_t* row_idx, const double* vals,
                       const double* col_lb, const double* col_ub, const double* row_lb,
                       const double* row_ub, const double* obj, double obj_offset,
                       double obj_scale, int32_t maximize, const volatile int32_t* interrupt,
                       mi_lp_result* out, double* primal, double* duals, double* reduced_costs,
                       double* activities, int8_t* var_status, int8_t* cons_status);

/* The same LPSolver flow with the simplex supplied by the caller
 * (LPSolver::RunRevisedSimplexIfNeeded, lp_solver.cc:591-658, is the call
 * site): fn receives the presolved and scaled LP, fills out (problem_status,
 * iterations, error_code) and the solution arrays (n primal values, m dual
 * values, n variable and m constraint statuses) and returns MI_LP_OK or an
 * error code, which is passed through. mi_lp_solver_solve is this with the
 * engine's handle behind fn. */
typedef int (*mi_lp_simplex_fn)(void* user, int32_t m, int32_t n, const int64_t* col_starts,
                                const int32_t* row_idx, const double* vals,
                                const double* col_lb, const double* col_ub,
                                const double* row_lb, const double* row_ub, const double* obj,
                                double obj_offset, double obj_scale, int32_t maximize,
                                mi_lp_result* out, double* primal, double* duals,
                                int8_t* var_status, int8_t* cons_status);
int mi_lp_solver_solve_with(mi_lp_simplex_fn fn, void* user, const mi_lp_solver_params* sp,
                            int32_t m, int32_t n, const int64_t* col_starts,
                            const int32_t* row_idx, const double* vals, const double* col_lb,
                            const double* col_ub, const double* row_lb, const double* row_ub,
                            const double* obj, double obj_offset, double obj_scale,
                            int32_t maximize, mi_lp_result* out, double* primal, double* duals,
                            double* reduced_costs, double* activities, int8_t* var_status,
                            int8_t* cons_status);

/* Presolve alone (host only, no device needed): MainLpPreprocessor's passes
 * (glop/preprocessor.cc:76-147, without the scaling) on a copy of the LP, and
 * DestructiveRecoverSolution (:203-209) for a solution of the presolved LP.
 *   mi_presolve_run       *status = Glop's status after presolve (MI_LP_INIT:
 *                         the simplex must run on the presolved LP;
 *                         MI_LP_INVALID_PROBLEM: IsValid failed, nothing ran)
 *   mi_presolve_dims      presolved sizes and direction (the dualizer turns
 *                         the LP into a maximization)
 *   mi_presolve_get       the presolved LP (any pointer may be NULL)
 *   mi_presolve_recover   solution of the presolved LP (its sizes) -> solution
 *                         of the original LP (original sizes); *status in/out
 *                         (the dualizer maps primal/dual statuses); once only
 *   mi_presolve_pass_name the passes that changed the LP, in order */
typedef struct mi_presolve mi_presolve;
mi_presolve* mi_presolve_create(void);
void mi_presolve_destroy(mi_presolve* ps);
int mi_presolve_run(mi_presolve* ps, const mi_lp_solver_params* sp, int32_t m, int32_t n,
                    const int64_t* col_starts, const int32_t* row_idx, const double* vals,
                    const double* col_lb, const double* col_ub, const double* row_lb,
                    const double* row_ub, const double* obj, double obj_offset, double obj_scale,
                    int32_t maximize, int32_t* status);
int mi_presolve_dims(const mi_presolve* ps, int32_t* m, int32_t* n, int64_t* nnz,
                     int32_t* maximize);
int mi_presolve_get(const mi_presolve* ps, int64_t* col_starts, int32_t* row_idx, double* vals,
                    double* col_lb, double* col_ub, double* row_lb, double* row_ub, double* obj,
                    double* obj_offset, double* obj_scale);
int mi_presolve_recover(mi_presolve* ps, int32_t* status, const double* primal,
                        const double* duals, const int8_t* var_status, const int8_t* cons_status,
                        double* primal_out, double* duals_out, int8_t* var_status_out,
                        int8_t* cons_status_out);
int32_t mi_presolve_num_passes(const mi_presolve* ps);
const char* mi_presolve_pass_name(const mi_presolve* ps, int32_t i);

#ifdef __cplusplus
}
#endif

#endif /* MI_LP_H_ */
