// The workspace of DeviceLp's panel calls (device_panel.hip): the buffers of
// ColumnDotsPanel, ColumnDotsPanelSparse, ColumnPenaltiesPanel,
// ColumnCutsPanel, RowSumsPanel, RowSumsPanelFrom,
// RowViolationsPanel(From), BoundRangesPanel(From),
// BoundInfeasiblePanel(From), BoundImpliedPanel(From),
// BoundTightenedPanel(From), BoundPropagatePanel(From) and
// BoundPropagatedColumnsFrom, their timing events and their test records.
// Included by the HIP translation units only; device_lp.h holds the workspace
// behind a pointer.
#ifndef MILP_DEVICE_PANEL_H_
#define MILP_DEVICE_PANEL_H_

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "../kernels/kernel_args.h"
#include "device_lp.h"

namespace milp {

inline void PanelCheck(hipError_t err, const char* what) {
  if (err != hipSuccess) throw DeviceError(std::string(what) + ": " + hipGetErrorString(err));
}

// A buffer that owns its memory, device or pinned host. Capacity counts
// elements of T and grows to exactly what is asked for; the contents are not
// kept across a growth. Freed with the buffer: the owner sees to it that the
// allocating device is current and no launch still uses the memory.
template <typename T, bool kPinned>
class PanelBuffer {
 public:
  PanelBuffer() = default;
  PanelBuffer(const PanelBuffer&) = delete;
  PanelBuffer& operator=(const PanelBuffer&) = delete;
  ~PanelBuffer() { (void)Free(); }

  T* Reserve(size_t count, const char* what) {
    if (count > capacity_) {
      PanelCheck(Free(), what);
      void* p = nullptr;
      PanelCheck(kPinned ? hipHostMalloc(&p, count * sizeof(T)) : hipMalloc(&p, count * sizeof(T)),
                 what);
      ptr_ = static_cast<T*>(p);
      capacity_ = count;
    }
    return ptr_;
  }
  T* get() const { return ptr_; }

 private:
  hipError_t Free() {
    T* p = ptr_;
    ptr_ = nullptr;
    capacity_ = 0;
    if (p == nullptr) return hipSuccess;
    return kPinned ? hipHostFree(p) : hipFree(p);
  }
  T* ptr_ = nullptr;
  size_t capacity_ = 0;
};
template <typename T>
using DeviceBuffer = PanelBuffer<T, false>;
template <typename T>
using PinnedBuffer = PanelBuffer<T, true>;

// Not in DeviceLp's allocations_: the workspace outlives a matrix upload,
// grows at first use and is freed with the handle. A panel has `width` (1, 4
// or 16) interleaved slots of which kp are in use; m rows, N columns.
struct PanelWorkspace {
  PanelWorkspace() = default;
  PanelWorkspace(const PanelWorkspace&) = delete;
  PanelWorkspace& operator=(const PanelWorkspace&) = delete;
  ~PanelWorkspace();

  // The three buffers both directions share (PanelReserve sizes them), and
  // what each direction keeps in them:
  //                                   column dots (y -> a_col . y)  row sums (x -> A x)
  //   rows: row-interleaved,          the vectors y                 the results
  //         max(1, m width)
  //   cols: column-interleaved,       the results                   the points x
  //         N width
  //   flat: vector-major, kp N        the results on their way      the points on their way
  //                                   down (sparse form: the        up, then the results
  //                                   packed kept values)           (kp m) on their way down
  // The Gomory cuts (ColumnCutsPanel) are column dots twice over: `rows`
  // holds rho, then the slack part of g; `cols` alpha, then s, then the cut
  // coefficients c over its first n columns (see cut_g below).
  // The row violations (RowViolationsPanel, RowViolationsPanelFrom) are row
  // sums up to the results in `rows`; then `flat` takes the packed kept
  // activities (at most kp m <= kp N), the points having left it.
  //
  // The bound sets' activity ranges (BoundRangesPanel(From),
  // BoundInfeasiblePanel(From)) are the row sums' direction with two point
  // arrays over the n structural columns: `cols` takes the interleaved lower
  // bounds and `cols_upper` (below) the upper bounds; `flat` takes both
  // arrays on their way up (2 kp n), `rows` the three result blocks lo, hi
  // and packed counts (3 m width) or, when screening, g alone (m width), and
  // `flat` then the results on their way down (3 kp m) or the packed kept
  // amounts. PanelReserve(ranges) sizes them for that.
  DeviceBuffer<double> rows, cols, flat;
  // Activity ranges only: the column-interleaved upper bounds, max(1, n)
  // width, read beside `cols` (the lower bounds) by the kernel.
  DeviceBuffer<double> cols_upper;
  // The implied column bounds (BoundImpliedPanel(From),
  // BoundTightenedPanel(From)) are an activity-range call in its dense mode
  // up to the three result blocks in `rows`, which stay there; `cols` and
  // `cols_upper` still hold the own bounds. implied_bounds_panel_kernel
  // writes three column-interleaved blocks of max(1, n) width into `implied`:
  // the new lower bounds, the new upper bounds and (filtered form) the keys.
  // `flat`, the sets having left it, takes three blocks of kp n: the dense
  // form's new lower and upper bounds on their way down, or the filtered
  // form's packed lower bounds, upper bounds and keys (kept_cols beside them).
  // PanelReserve(ranges, implied) sizes them for that. row_lb / row_ub and,
  // in the override form, base / base_upper are read as uploaded.
  //
  // The bound propagation (BoundPropagatePanel(From),
  // BoundPropagatedColumnsFrom) repeats that per round on the same buffers:
  // `rows` takes the round's ranges, `implied`'s first two blocks the round's
  // implied bounds, and propagate_apply_panel_kernel moves the own bounds in
  // `cols` / `cols_upper` IN PLACE, writes the round's keys into the third
  // block and, in round 1, move-only keys into a fourth
  // (PanelReserve(ranges, implied, propagate) sizes `implied` at four blocks).
  // `is_integer` (below) is read as uploaded. After the rounds `flat` takes
  // the final bounds on their way down, two blocks of kp n, or the packed
  // kept bounds and keys as for the tightened columns, whose keys
  // propagate_changed_keys_kernel writes into the third block of `implied`.
  DeviceBuffer<double> implied;
  DeviceBuffer<uint8_t> is_integer;  // the propagation only: n, uploaded once per call
  PinnedBuffer<double> y_staging;  // column dots: the host interleave of y, max(1, m width)

  // ColumnDotsPanelSparse and the row violations: tiles of 256 columns
  // (sparse rows) or 256 rows (violations).
  DeviceBuffer<int32_t> kept_cols;   // packed kept columns, N kp / kept rows, at most m kp
  DeviceBuffer<uint64_t> keep_mask;  // ceil(N / 64) words (sparse rows only)
  DeviceBuffer<int> counts;          // kp x tiles
  DeviceBuffer<int64_t> offsets;     // kp x tiles, then kPanelMaxWidth totals
  PinnedBuffer<int64_t> totals;      // kPanelMaxWidth

  // The row violations only.
  DeviceBuffer<double> row_lb, row_ub;    // the bounds, m each, uploaded once per call
  DeviceBuffer<double> tile_worst;        // kp x tiles: largest amount of (point, tile)
  DeviceBuffer<int32_t> tile_worst_row;   // kp x tiles: lowest row attaining it
  DeviceBuffer<milp_kernels::PointViolations> summaries;       // kPanelMaxWidth
  PinnedBuffer<milp_kernels::PointViolations> summaries_host;  // kPanelMaxWidth

  // ColumnPenaltiesPanel only: column dots up to the results in `cols`, which
  // penalties_tile / penalties_fold reduce; `flat` is not used. The per-tile
  // partials of both directions go into tile_worst (minima), tile_worst_row
  // (columns) and counts, 2 kp x tiles each (tiles of 256 columns).
  DeviceBuffer<double> penalty_d;        // reduced costs, N, uploaded once per call
  DeviceBuffer<uint8_t> penalty_status;  // N, uploaded once per call
  DeviceBuffer<double> penalty_unit;     // integer steps, N, uploaded once per call (if given)
  DeviceBuffer<double> penalty_dist;     // down distances (k), then up (k), once per call
  DeviceBuffer<milp_kernels::BranchPenalty> penalties;       // kPanelMaxWidth
  PinnedBuffer<milp_kernels::BranchPenalty> penalties_host;  // kPanelMaxWidth

  // ColumnCutsPanel only: column dots up to the results (alpha) in `cols`.
  // gomory_transform_tile writes g of the structural columns into `cut_g` and
  // g of slack column n + r over rho in `rows` (row-interleaved: the vector
  // y' of the second dot pass, zero in the padding slots); the dot kernels
  // run again and leave s in `cols`; gomory_combine_tile writes c = g - s
  // over the first n columns of `cols` in place, where the sparse form's
  // passes then read it as a panel result of n columns (`flat` takes the
  // packed kept values, kept_cols / counts / offsets / totals as for the
  // sparse rows). The per-tile partials: tile_worst takes the largest and
  // then the smallest fabs(c) (2 kp x structural tiles), tile_worst_row the
  // columns attaining them likewise, cut_counts the bad columns (kp x tiles
  // over N), then the kept and the NaN counts (kp x structural tiles each).
  // penalty_status and penalty_unit take the statuses and steps.
  DeviceBuffer<double> cut_g;       // max(1, n) width, column-interleaved
  DeviceBuffer<double> cut_vector;  // f0 (k), then row_unit (k), once per call
  DeviceBuffer<int> cut_counts;
  DeviceBuffer<milp_kernels::CutSummary> cut_summaries;       // kPanelMaxWidth
  PinnedBuffer<milp_kernels::CutSummary> cut_summaries_host;  // kPanelMaxWidth

  // RowSumsPanelFrom and RowViolationsPanelFrom, uploaded once per call.
  DeviceBuffer<double> base;        // the base point, N
  DeviceBuffer<int64_t> ov_starts;  // k + 1
  DeviceBuffer<int32_t> ov_cols;    // overrides of the whole call
  DeviceBuffer<double> ov_vals;
  // BoundRangesPanelFrom and BoundInfeasiblePanelFrom: the upper bounds'
  // base (n) and override values beside the lower bounds' in base / ov_vals.
  DeviceBuffer<double> base_upper;
  DeviceBuffer<double> ov_vals_upper;

  // Kernel time (TakePanelKernelMs): off until the first take.
  bool timing = false;
  double kernel_ms = 0.0;
  hipEvent_t ev[2] = {nullptr, nullptr};  // created by the first timed panel

  DeviceLp::LastPanel last_panel;
  DeviceLp::LastPanelSparse last_panel_sparse;
  DeviceLp::LastPenalties last_penalties;
  DeviceLp::LastCuts last_cuts;
  DeviceLp::LastRowPanel last_row_panel;
  DeviceLp::LastRowViolations last_row_violations;
  DeviceLp::LastBoundRanges last_bound_ranges;
  DeviceLp::LastBoundImplied last_bound_implied;
  DeviceLp::LastBoundPropagate last_bound_propagate;
};

}  // namespace milp

#endif  // MILP_DEVICE_PANEL_H_
