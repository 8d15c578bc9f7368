// DeviceLp's panel calls: k vectors per pass over [A | I] (see device_lp.h).
// Column dots (ColumnDotsPanel, ColumnDotsPanelSparse, their reduction to
// branching penalties, ColumnPenaltiesPanel, and the Gomory cuts built from
// two passes of them, ColumnCutsPanel), row sums (RowSumsPanel,
// RowSumsPanelFrom), their violated rows (RowViolationsPanel,
// RowViolationsPanelFrom) and the activity ranges of bound sets
// (BoundRangesPanel(From), BoundInfeasiblePanel(From)) with the implied column
// bounds over them (BoundImpliedPanel(From), BoundTightenedPanel(From)) and
// their rounds to a fixpoint (BoundPropagatePanel(From),
// BoundPropagatedColumnsFrom) share
// one workspace (device_panel.h), one panel loop and one timing scope. No
// solve calls them and nothing a solve reads is written.
#include "device_panel.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../kernels/kernel_args.h"

namespace milp {

namespace {
inline hipStream_t S(void* p) { return reinterpret_cast<hipStream_t>(p); }

int PanelWidth(int kp) { return kp == 1 ? 1 : (kp <= 4 ? 4 : 16); }

// body(first, kp, width) for the k vectors in panels of up to kPanelMaxWidth.
template <typename Body>
void ForEachPanel(int k, Body body) {
  for (int first = 0; first < k; first += milp_kernels::kPanelMaxWidth) {
    const int kp = std::min(milp_kernels::kPanelMaxWidth, k - first);
    body(first, kp, PanelWidth(kp));
  }
}
}  // namespace

// The kernel time of one panel, when the workspace's timing is on: starts
// where it is constructed, Launched() after the panel's last launch,
// Downloaded() after the synchronizing download that follows.
class PanelTimer {
 public:
  PanelTimer(PanelWorkspace* w, hipStream_t stream) : w_(w), stream_(stream) {
    if (!w_->timing) return;
    for (hipEvent_t& e : w_->ev) {
      if (e == nullptr) PanelCheck(hipEventCreate(&e), "hipEventCreate");
    }
    PanelCheck(hipEventRecord(w_->ev[0], stream_), "ev");
  }
  void Launched() {
    if (w_->timing) PanelCheck(hipEventRecord(w_->ev[1], stream_), "ev");
  }
  void Downloaded() {
    if (!w_->timing) return;
    float ms = 0.0f;
    PanelCheck(hipEventElapsedTime(&ms, w_->ev[0], w_->ev[1]), "ev time");
    w_->kernel_ms += ms;
  }
  // A panel with more than one synchronizing download (the rounds of the
  // bound propagation): after Downloaded(), the next stretch starts here.
  void Restart() {
    if (w_->timing) PanelCheck(hipEventRecord(w_->ev[0], stream_), "ev");
  }

 private:
  PanelWorkspace* w_;
  hipStream_t stream_;
};

PanelWorkspace::~PanelWorkspace() {
  for (hipEvent_t e : ev) {
    if (e != nullptr) (void)hipEventDestroy(e);
  }
}

DeviceLp::DeviceLp() : panel_(new PanelWorkspace) {}

DeviceLp::LastPanel DeviceLp::last_panel() const { return panel_->last_panel; }
DeviceLp::LastPanelSparse DeviceLp::last_panel_sparse() const { return panel_->last_panel_sparse; }
DeviceLp::LastRowPanel DeviceLp::last_row_panel() const { return panel_->last_row_panel; }

double DeviceLp::TakePanelKernelMs() {
  double ms = panel_->kernel_ms;
  panel_->kernel_ms = 0.0;
  panel_->timing = true;
  for (auto& d : shards_) {
    if (d) ms += d->TakePanelKernelMs();
  }
  return ms;
}

int DeviceLp::PanelTileColumns() { return milp_kernels::kPanelTileColumns; }
int DeviceLp::PanelOffsetsStepTiles() { return milp_kernels::kPanelOffsetsStep; }

void DeviceLp::RowPanelGeometry(int rows_per_workgroup[3], int* chunk) {
  rows_per_workgroup[0] = milp_kernels::kRowPanelThreads;
  rows_per_workgroup[1] = milp_kernels::kRowPanelThreads / 4;
  rows_per_workgroup[2] = milp_kernels::kRowPanelThreads / 16;
  *chunk = milp_kernels::kRowPanelChunk;
}

// Grows the three shared buffers to one panel of `width` holding `kp`
// vectors. The stream is idle between panels (each ends with a synchronizing
// download).
// ranges, implied, propagate: the roles of the activity ranges, of the implied
// column bounds over them and of the propagation's rounds (device_panel.h).
void DeviceLp::PanelReserve(int width, int kp, bool ranges, bool implied, bool propagate) {
  const size_t n = size_t(n_total_ - m_);
  size_t rows = size_t(m_) * width;
  size_t flat = size_t(n_total_) * kp;
  if (ranges) {
    rows *= 3;
    flat = std::max(flat, std::max(2 * n, 3 * size_t(m_)) * kp);
    // At least one column: the kernel redirects a slack's gather to column 0.
    panel_->cols_upper.Reserve(std::max<size_t>(1, n) * width, "panel upper bounds");
  }
  if (implied) {
    flat = std::max(flat, 3 * n * kp);
    panel_->implied.Reserve((propagate ? 4 : 3) * std::max<size_t>(1, n) * width,
                            "panel implied bounds");
  }
  panel_->rows.Reserve(std::max<size_t>(1, rows), "panel rows");
  panel_->cols.Reserve(size_t(n_total_) * width, "panel columns");
  panel_->flat.Reserve(flat, "panel vector-major");
}

DeviceLp::PanelPlan DeviceLp::PanelKernelChoice() const {
  PanelPlan plan;
  const double sparse_avg =
      (nd_ > 0 ? (ns_ > 0 ? double(sparse_entries_) / ns_ : 0.0) : avg_col_len_);
  plan.long_columns = sparse_avg >= 32.0;  // LaunchColumnDots' rule
  plan.sparse_cols = nd_ > 0 ? ns_ : n_total_;
  return plan;
}

// Vectors [first, first + kp) of y, interleaved on the host, into `rows`.
void DeviceLp::PanelUploadVectors(const double* y, int first, int kp, int width) {
  PanelReserve(width, kp);
  double* staging =
      panel_->y_staging.Reserve(std::max<size_t>(1, size_t(m_) * width), "panel staging");
  for (int r = 0; r < m_; ++r) {
    double* dst = staging + size_t(r) * width;
    for (int v = 0; v < kp; ++v) dst[v] = y[size_t(first + v) * m_ + r];
    for (int v = kp; v < width; ++v) dst[v] = 0.0;
  }
  Upload(panel_->rows.get(), staging, size_t(m_) * width * sizeof(double));
}

// The dots of every column with the vectors in `rows`, into `cols`.
void DeviceLp::PanelLaunchDots(const PanelPlan& plan, int kp, int width) {
  milp_kernels::PanelDotArgs a{};
  a.starts = d_starts_;
  a.rows = d_rows_;
  a.vals = d_vals_;
  a.y = panel_->rows.get();
  a.ncols = plan.sparse_cols;
  a.col_list = nd_ > 0 ? d_sparse_cols_ : nullptr;
  a.kp = kp;
  a.out = panel_->cols.get();
  Check(milp_launch::column_dot_panel(width, plan.long_columns, a, S(stream_)),
        "column dots panel");
  if (nd_ > 0) {
    milp_kernels::PanelDenseArgs d{};
    d.body = d_dense_body_;
    d.tail = d_dense_tail_;
    d.dense_cols = d_dense_cols_;
    d.nd = nd_;
    d.m = m_;
    d.y = panel_->rows.get();
    d.kp = kp;
    d.out = panel_->cols.get();
    Check(milp_launch::dense_dot_panel(width, d, S(stream_)), "dense dots panel");
  }
}

void DeviceLp::PanelRecord(const PanelPlan& plan, int width, LastPanel* record) const {
  record->sparse = plan.sparse_cols > 0
                       ? (plan.long_columns ? kPanelLongColumns : kPanelShortColumns)
                       : kPanelNone;
  record->dense = nd_ > 0;
  record->panels += 1;
  record->width = width;
}

void DeviceLp::ColumnDotsPanel(const double* y, int k, double* out) {
  if (!shards_.empty()) return ShardedColumnDotsPanel(y, k, out);
  PanelWorkspace& w = *panel_;
  w.last_panel = LastPanel();
  if (k <= 0 || n_total_ <= 0) return;
  DeviceOp("column dots panel");
  const PanelPlan plan = PanelKernelChoice();
  ForEachPanel(k, [&](int first, int kp, int width) {
    PanelUploadVectors(y, first, kp, width);
    PanelTimer timer(&w, S(stream_));
    PanelLaunchDots(plan, kp, width);
    Check(milp_launch::panel_deinterleave(width, w.cols.get(), n_total_, kp, w.flat.get(),
                                          n_total_, S(stream_)),
          "panel de-interleave");
    timer.Launched();
    Download(out + size_t(first) * n_total_, w.flat.get(),
             size_t(kp) * n_total_ * sizeof(double));
    timer.Downloaded();
    PanelRecord(plan, width, &w.last_panel);
  });
  DeviceOp("column dots panel done");
}

void DeviceLp::ColumnDotsPanelSparse(const double* y, int k, double drop_tolerance,
                                     const uint64_t* keep_words, SparseRows* out) {
  if (!shards_.empty()) {
    return ShardedColumnDotsPanelSparse(y, k, drop_tolerance, keep_words, out);
  }
  PanelWorkspace& w = *panel_;
  w.last_panel_sparse = LastPanelSparse();
  out->row_starts.assign(size_t(std::max(k, 0)) + 1, 0);
  out->cols.clear();
  out->vals.clear();
  if (k <= 0 || n_total_ <= 0) return;
  DeviceOp("column dots panel sparse");
  const PanelPlan plan = PanelKernelChoice();
  const int tiles = (n_total_ + milp_kernels::kPanelTileColumns - 1) /
                    milp_kernels::kPanelTileColumns;
  const size_t mask_words = size_t((n_total_ + 63) / 64);
  ForEachPanel(k, [&](int first, int kp, int width) {
    PanelUploadVectors(y, first, kp, width);
    PanelTimer timer(&w, S(stream_));
    PanelLaunchDots(plan, kp, width);
    // The sparse form's own buffers; `flat` takes the packed values.
    w.kept_cols.Reserve(size_t(n_total_) * kp, "panel kept columns");
    w.keep_mask.Reserve(mask_words, "panel mask");
    w.counts.Reserve(size_t(kp) * tiles, "panel counts");
    w.offsets.Reserve(size_t(kp) * tiles + milp_kernels::kPanelMaxWidth, "panel offsets");
    const int64_t* totals = w.totals.Reserve(milp_kernels::kPanelMaxWidth, "panel totals");
    if (first == 0 && keep_words != nullptr) {
      Upload(w.keep_mask.get(), keep_words, mask_words * sizeof(uint64_t));
    }
    milp_kernels::PanelSparseArgs a{};
    a.in = w.cols.get();
    a.ncols = n_total_;
    a.kp = kp;
    a.tiles = tiles;
    a.mask = keep_words != nullptr ? w.keep_mask.get() : nullptr;
    a.drop_tolerance = drop_tolerance;
    a.counts = w.counts.get();
    a.offsets = w.offsets.get();
    a.totals = w.offsets.get() + size_t(kp) * tiles;
    a.cols = w.kept_cols.get();
    a.vals = w.flat.get();
    Check(milp_launch::panel_sparse(width, a, S(stream_)), "panel sparse rows");
    timer.Launched();
    // Down: the kp totals, then exactly the kept entries.
    Download(w.totals.get(), a.totals, size_t(kp) * sizeof(int64_t));
    int64_t kept = 0;
    for (int v = 0; v < kp; ++v) {
      if (totals[v] < 0 || totals[v] > n_total_) {
        throw DeviceError("panel sparse rows: bad count");
      }
      kept += totals[v];
      out->row_starts[first + v + 1] = out->row_starts[first + v] + totals[v];
    }
    const size_t old = out->cols.size();
    out->cols.resize(old + size_t(kept));
    out->vals.resize(old + size_t(kept));
    if (kept > 0) {
      Check(hipMemcpyAsync(out->cols.data() + old, a.cols, size_t(kept) * sizeof(int32_t),
                           hipMemcpyDeviceToHost, S(stream_)),
            "D2H");
      Download(out->vals.data() + old, a.vals, size_t(kept) * sizeof(double));
    }
    timer.Downloaded();
    PanelRecord(plan, width, &w.last_panel_sparse.panel);
    w.last_panel_sparse.kept += kept;
    w.last_panel_sparse.bytes_down += int64_t(kp) * 8 + kept * 12;
  });
  DeviceOp("column dots panel sparse done");
}

static_assert(sizeof(milp_kernels::BranchPenalty) == sizeof(mi_lp_branch_penalty) &&
                  sizeof(mi_lp_branch_penalty) == 32 &&
                  offsetof(milp_kernels::BranchPenalty, up) == offsetof(mi_lp_branch_penalty, up) &&
                  offsetof(milp_kernels::BranchPenalty, down_col) ==
                      offsetof(mi_lp_branch_penalty, down_col) &&
                  offsetof(milp_kernels::BranchPenalty, up_count) ==
                      offsetof(mi_lp_branch_penalty, up_count),
              "kernel_args.h restates mi_lp_branch_penalty");

DeviceLp::LastPenalties DeviceLp::last_penalties() const { return panel_->last_penalties; }

bool DeviceLp::ValidPenaltyArgs(int num_cols, int k, const int8_t* status, const double* unit,
                                const double* down_dist, const double* up_dist,
                                double pivot_tolerance) {
  if (k < 0 || !(pivot_tolerance >= 0.0)) return false;
  auto distance = [](double x) { return x >= 0.0 && x < HUGE_VAL; };  // false for a NaN
  for (int j = 0; j < k; ++j) {
    if (!distance(down_dist[j]) || !distance(up_dist[j])) return false;
  }
  for (int c = 0; c < num_cols; ++c) {
    if (status[c] < MI_LP_BASIC || status[c] > MI_LP_FREE) return false;
    if (unit != nullptr && !distance(unit[c])) return false;
  }
  return true;
}

void DeviceLp::ColumnPenaltiesPanel(const double* y, int k, const double* d,
                                    const uint8_t* status, const double* unit,
                                    const double* down_dist, const double* up_dist,
                                    double pivot_tolerance, mi_lp_branch_penalty* out) {
  if (!shards_.empty()) {
    return ShardedColumnPenaltiesPanel(y, k, d, status, unit, down_dist, up_dist,
                                       pivot_tolerance, out);
  }
  PanelWorkspace& w = *panel_;
  w.last_penalties = LastPenalties();
  for (int j = 0; j < k; ++j) {
    out[j] = mi_lp_branch_penalty{HUGE_VAL, HUGE_VAL, -1, -1, 0, 0};
  }
  if (k <= 0 || n_total_ <= 0) return;
  DeviceOp("column penalties panel");
  const PanelPlan plan = PanelKernelChoice();
  const int tiles = (n_total_ + milp_kernels::kPanelTileColumns - 1) /
                    milp_kernels::kPanelTileColumns;
  const size_t N = size_t(n_total_);
  Upload(w.penalty_d.Reserve(N, "panel reduced costs"), d, N * sizeof(double));
  Upload(w.penalty_status.Reserve(N, "panel statuses"), status, N);
  if (unit != nullptr) {
    Upload(w.penalty_unit.Reserve(N, "panel integer steps"), unit, N * sizeof(double));
  }
  double* dist = w.penalty_dist.Reserve(2 * size_t(k), "panel distances");
  Upload(dist, down_dist, size_t(k) * sizeof(double));
  Upload(dist + k, up_dist, size_t(k) * sizeof(double));
  w.last_penalties.tiles = tiles;
  ForEachPanel(k, [&](int first, int kp, int width) {
    PanelUploadVectors(y, first, kp, width);
    PanelTimer timer(&w, S(stream_));
    PanelLaunchDots(plan, kp, width);
    const size_t partials = 2 * size_t(kp) * tiles;
    milp_kernels::PenaltyArgs a{};
    a.in = w.cols.get();
    a.ncols = n_total_;
    a.kp = kp;
    a.tiles = tiles;
    a.d = w.penalty_d.get();
    a.status = w.penalty_status.get();
    a.unit = unit != nullptr ? w.penalty_unit.get() : nullptr;
    a.down_dist = dist + first;
    a.up_dist = dist + k + first;
    a.pivot_tolerance = pivot_tolerance;
    a.tile_min = w.tile_worst.Reserve(partials, "panel tile minima");
    a.tile_col = w.tile_worst_row.Reserve(partials, "panel tile columns");
    a.tile_count = w.counts.Reserve(partials, "panel counts");
    a.out = w.penalties.Reserve(milp_kernels::kPanelMaxWidth, "panel penalties");
    const milp_kernels::BranchPenalty* host =
        w.penalties_host.Reserve(milp_kernels::kPanelMaxWidth, "panel penalties");
    Check(milp_launch::panel_penalties(width, a, S(stream_)), "panel penalties");
    timer.Launched();
    Download(w.penalties_host.get(), a.out, size_t(kp) * sizeof(*a.out));
    timer.Downloaded();
    for (int v = 0; v < kp; ++v) {
      const milp_kernels::BranchPenalty& p = host[v];
      if (p.down_count < 0 || p.down_count > n_total_ || p.up_count < 0 ||
          p.up_count > n_total_ || p.down_col < -1 || p.down_col >= n_total_ ||
          p.up_col < -1 || p.up_col >= n_total_) {
        throw DeviceError("column penalties panel: bad record");
      }
      out[first + v] =
          mi_lp_branch_penalty{p.down, p.up, p.down_col, p.up_col, p.down_count, p.up_count};
    }
    PanelRecord(plan, width, &w.last_penalties.panel);
    w.last_penalties.bytes_down += int64_t(kp) * 32;
  });
  DeviceOp("column penalties panel done");
}

static_assert(sizeof(milp_kernels::CutSummary) == sizeof(mi_lp_cut_summary) &&
                  sizeof(mi_lp_cut_summary) == 32 &&
                  offsetof(milp_kernels::CutSummary, min_abs) ==
                      offsetof(mi_lp_cut_summary, min_abs) &&
                  offsetof(milp_kernels::CutSummary, count) == offsetof(mi_lp_cut_summary, count) &&
                  offsetof(milp_kernels::CutSummary, bad_count) ==
                      offsetof(mi_lp_cut_summary, bad_count) &&
                  offsetof(milp_kernels::CutSummary, min_col) ==
                      offsetof(mi_lp_cut_summary, min_col),
              "kernel_args.h restates mi_lp_cut_summary");

DeviceLp::LastCuts DeviceLp::last_cuts() const { return panel_->last_cuts; }

bool DeviceLp::ValidCutArgs(int num_cols, int k, const int8_t* status, const double* unit,
                            const double* f0, const double* row_unit, double zero_tolerance,
                            double drop_tolerance) {
  if (k < 0 || !(zero_tolerance >= 0.0) || !(zero_tolerance < HUGE_VAL) ||
      !(drop_tolerance >= 0.0)) {
    return false;
  }
  for (int j = 0; j < k; ++j) {  // every comparison is false for a NaN
    if (!(f0[j] > 0.0 && f0[j] < 1.0)) return false;
    if (!(row_unit[j] > 0.0 && row_unit[j] < HUGE_VAL)) return false;
  }
  for (int c = 0; c < num_cols; ++c) {
    if (status[c] < MI_LP_BASIC || status[c] > MI_LP_FREE) return false;
    if (unit != nullptr && !(unit[c] >= 0.0 && unit[c] < HUGE_VAL)) return false;
  }
  return true;
}

void DeviceLp::ColumnCutsPanel(const double* y, int k, const uint8_t* status, const double* unit,
                               const double* f0, const double* row_unit, double zero_tolerance,
                               double drop_tolerance, bool lists, CutRows* out) {
  if (!shards_.empty()) throw DeviceError("column cuts panel: not with column shards");
  PanelWorkspace& w = *panel_;
  w.last_cuts = LastCuts();
  w.last_cuts.lists = lists;
  out->row_starts.clear();
  if (lists) out->row_starts.assign(size_t(std::max(k, 0)) + 1, 0);
  out->cols.clear();
  out->vals.clear();
  out->summaries.assign(size_t(std::max(k, 0)), mi_lp_cut_summary{0.0, HUGE_VAL, 0, 0, -1, -1});
  if (k <= 0 || n_total_ <= 0) return;
  DeviceOp("column cuts panel");
  const PanelPlan plan = PanelKernelChoice();
  const int n = n_total_ - m_;
  const int tiles = (n_total_ + milp_kernels::kPanelTileColumns - 1) /
                    milp_kernels::kPanelTileColumns;
  const int tiles_n = (n + milp_kernels::kPanelTileColumns - 1) / milp_kernels::kPanelTileColumns;
  const size_t N = size_t(n_total_);
  Upload(w.penalty_status.Reserve(N, "panel statuses"), status, N);
  if (unit != nullptr) {
    Upload(w.penalty_unit.Reserve(N, "panel integer steps"), unit, N * sizeof(double));
  }
  double* per_vector = w.cut_vector.Reserve(2 * size_t(k), "panel cut vectors");
  Upload(per_vector, f0, size_t(k) * sizeof(double));
  Upload(per_vector + k, row_unit, size_t(k) * sizeof(double));
  w.last_cuts.tiles = tiles;
  w.last_cuts.structural_tiles = tiles_n;
  ForEachPanel(k, [&](int first, int kp, int width) {
    PanelUploadVectors(y, first, kp, width);
    PanelTimer timer(&w, S(stream_));
    PanelLaunchDots(plan, kp, width);
    const size_t part_n = size_t(kp) * tiles_n;
    milp_kernels::GomoryArgs a{};
    a.cols = w.cols.get();
    a.g = w.cut_g.Reserve(std::max<size_t>(1, size_t(n)) * width, "panel cut coefficients");
    a.slack = w.rows.get();
    a.ncols = n_total_;
    a.n = n;
    a.kp = kp;
    a.tiles = tiles;
    a.tiles_n = tiles_n;
    a.status = w.penalty_status.get();
    a.unit = unit != nullptr ? w.penalty_unit.get() : nullptr;
    a.f0 = per_vector + first;
    a.row_unit = per_vector + k + first;
    a.zero_tolerance = zero_tolerance;
    a.drop_tolerance = drop_tolerance;
    a.tile_bad = w.cut_counts.Reserve(size_t(kp) * tiles + 2 * part_n, "panel cut counts");
    a.tile_count = a.tile_bad + size_t(kp) * tiles;
    a.tile_nan = a.tile_count + part_n;
    a.tile_max = w.tile_worst.Reserve(std::max<size_t>(1, 2 * part_n), "panel tile extrema");
    a.tile_min = a.tile_max + part_n;
    a.tile_max_col =
        w.tile_worst_row.Reserve(std::max<size_t>(1, 2 * part_n), "panel tile columns");
    a.tile_min_col = a.tile_max_col + part_n;
    a.out = w.cut_summaries.Reserve(milp_kernels::kPanelMaxWidth, "panel cut summaries");
    const milp_kernels::CutSummary* host =
        w.cut_summaries_host.Reserve(milp_kernels::kPanelMaxWidth, "panel cut summaries");
    Check(milp_launch::panel_gomory_transform(width, a, S(stream_)), "panel cut transform");
    PanelLaunchDots(plan, kp, width);  // y' = the slack part of g, in `rows`
    Check(milp_launch::panel_gomory_combine(width, a, S(stream_)), "panel cut combine");
    milp_kernels::PanelSparseArgs sp{};
    const int64_t* totals = nullptr;
    const bool pack = lists && n > 0;
    if (pack) {
      // The sparse form over the first n columns of `cols`; `flat` takes the
      // packed values.
      w.kept_cols.Reserve(size_t(n) * kp, "panel kept columns");
      w.counts.Reserve(part_n, "panel counts");
      w.offsets.Reserve(part_n + milp_kernels::kPanelMaxWidth, "panel offsets");
      totals = w.totals.Reserve(milp_kernels::kPanelMaxWidth, "panel totals");
      sp.in = w.cols.get();
      sp.ncols = n;
      sp.kp = kp;
      sp.tiles = tiles_n;
      sp.mask = nullptr;
      sp.drop_tolerance = drop_tolerance;
      sp.counts = w.counts.get();
      sp.offsets = w.offsets.get();
      sp.totals = w.offsets.get() + part_n;
      sp.cols = w.kept_cols.get();
      sp.vals = w.flat.get();
      Check(milp_launch::panel_sparse(width, sp, S(stream_)), "panel cut rows");
    }
    timer.Launched();
    if (pack) {
      Check(hipMemcpyAsync(w.totals.get(), sp.totals, size_t(kp) * sizeof(int64_t),
                           hipMemcpyDeviceToHost, S(stream_)),
            "D2H");
    }
    Download(w.cut_summaries_host.get(), a.out, size_t(kp) * sizeof(*a.out));
    int64_t kept = 0;
    for (int v = 0; v < kp; ++v) {
      const milp_kernels::CutSummary& s = host[v];
      if (s.count < 0 || s.count > n || s.bad_count < 0 || s.max_col < -1 || s.max_col >= n ||
          s.min_col < -1 || s.min_col >= n || (pack && totals[v] != s.count)) {
        throw DeviceError("column cuts panel: bad summary");
      }
      out->summaries[first + v] =
          mi_lp_cut_summary{s.max_abs, s.min_abs, s.count, s.bad_count, s.max_col, s.min_col};
      if (lists) {
        kept += s.count;
        out->row_starts[first + v + 1] = out->row_starts[first + v] + s.count;
      }
    }
    if (kept > 0) {
      const size_t old = out->cols.size();
      out->cols.resize(old + size_t(kept));
      out->vals.resize(old + size_t(kept));
      Check(hipMemcpyAsync(out->cols.data() + old, sp.cols, size_t(kept) * sizeof(int32_t),
                           hipMemcpyDeviceToHost, S(stream_)),
            "D2H");
      Download(out->vals.data() + old, sp.vals, size_t(kept) * sizeof(double));
    }
    timer.Downloaded();
    PanelRecord(plan, width, &w.last_cuts.panel);
    w.last_cuts.kept += kept;
    w.last_cuts.bytes_down += int64_t(kp) * 32 + (pack ? int64_t(kp) * 8 : 0) + kept * 12;
  });
  DeviceOp("column cuts panel done");
}

bool DeviceLp::ValidOverrides(int num_cols, int k, const int64_t* starts, const int32_t* cols) {
  if (k < 0 || starts[0] != 0) return false;
  for (int j = 0; j < k; ++j) {
    if (starts[j + 1] < starts[j]) return false;
  }
  if (starts[k] == 0) return true;
  if (cols == nullptr) return false;
  std::vector<int32_t> stamp(size_t(std::max(num_cols, 0)), 0);  // point + 1 that last set it
  for (int j = 0; j < k; ++j) {
    for (int64_t i = starts[j]; i < starts[j + 1]; ++i) {
      const int32_t c = cols[i];
      if (c < 0 || c >= num_cols || stamp[c] == j + 1) return false;
      stamp[c] = j + 1;
    }
  }
  return true;
}

void DeviceLp::PanelLaunchRanges(int kp, int width, bool screening) {
  PanelWorkspace& w = *panel_;
  milp_kernels::ActivityRangeArgs a{};
  a.t_starts = d_t_starts_;
  a.t_cols = d_t_cols_;
  a.t_vals = d_t_vals_;
  a.lower = w.cols.get();
  a.upper = w.cols_upper.get();
  a.num_rows = m_;
  a.num_structural = n_total_ - m_;
  a.kp = kp;
  if (screening) {  // g alone
    a.row_lb = w.row_lb.get();
    a.row_ub = w.row_ub.get();
  }
  a.out = w.rows.get();
  Check(milp_launch::activity_ranges_panel(width, a, S(stream_)), "activity ranges panel");
}

// The interleaved points of one panel are in `cols`: the sums into `rows`;
// then the dense form (vector-major into `flat`, down to sink.sums, and the
// record) or the violations form.
void DeviceLp::RowPanelSums(int first, int kp, int width, PanelTimer* timer,
                            const RowPanelSink& sink) {
  PanelWorkspace& w = *panel_;
  if (sink.propagate != nullptr) return RowPanelPropagate(first, kp, width, timer, sink);
  if (sink.ranges) {
    PanelLaunchRanges(kp, width, sink.violations != nullptr);
  } else {
    milp_kernels::RowPanelArgs a{};
    a.t_starts = d_t_starts_;
    a.t_cols = d_t_cols_;
    a.t_vals = d_t_vals_;
    a.x = w.cols.get();
    a.num_rows = m_;
    a.kp = kp;
    a.out = w.rows.get();
    Check(milp_launch::row_sums_panel(width, a, S(stream_)), "row sums panel");
  }
  if (sink.implied) return RowPanelImplied(first, kp, width, timer, sink);
  if (sink.violations != nullptr) return RowPanelViolations(first, kp, width, timer, sink);
  // The dense form: the result blocks of `rows` (one of sums; lo, hi and the
  // packed counts of ranges), each m x width, go vector-major into `flat`.
  const size_t block = size_t(m_) * width;
  const size_t down = size_t(kp) * m_;
  const int blocks = !sink.ranges ? 1 : (sink.inf_counts != nullptr ? 3 : 2);
  for (int b = 0; b < blocks; ++b) {
    Check(milp_launch::panel_deinterleave(width, w.rows.get() + b * block, m_, kp,
                                          w.flat.get() + b * down, m_, S(stream_)),
          "row panel de-interleave");
  }
  timer->Launched();
  if (sink.ranges) {
    Check(hipMemcpyAsync(sink.max_activity + size_t(first) * m_, w.flat.get() + down,
                         down * sizeof(double), hipMemcpyDeviceToHost, S(stream_)),
          "D2H");
    if (sink.inf_counts != nullptr) {
      // A packed pair lo_inf | hi_inf << 32 is the two int32 of the caller.
      Check(hipMemcpyAsync(sink.inf_counts + size_t(first) * m_ * 2, w.flat.get() + 2 * down,
                           down * sizeof(double), hipMemcpyDeviceToHost, S(stream_)),
            "D2H");
    }
  }
  Download(sink.sums + size_t(first) * m_, w.flat.get(), down * sizeof(double));
  timer->Downloaded();
  if (sink.ranges) {
    w.last_bound_ranges.panels += 1;
    w.last_bound_ranges.width = width;
    w.last_bound_ranges.bytes_down += int64_t(blocks) * int64_t(down) * 8;
    return;
  }
  w.last_row_panel.panels += 1;
  w.last_row_panel.width = width;
  w.last_row_panel.kernel = kRowPanelDirect;
}

// The k dense points, panel by panel: up vector-major, interleaved on the
// device, then RowPanelSums.
// A ranges call brings two arrays over the n structural columns: both go up
// into `flat`, one behind the other, and each is interleaved into its buffer.
void DeviceLp::RowPanels(const double* x, const double* upper, int k, const RowPanelSink& sink) {
  PanelWorkspace& w = *panel_;
  const int ncols = sink.ranges ? n_total_ - m_ : n_total_;
  ForEachPanel(k, [&](int first, int kp, int width) {
    PanelReserve(width, kp, sink.ranges, sink.implied, sink.propagate != nullptr);
    const size_t up = size_t(kp) * ncols;
    Upload(w.flat.get(), x + size_t(first) * ncols, up * sizeof(double));
    if (sink.ranges) Upload(w.flat.get() + up, upper + size_t(first) * ncols, up * sizeof(double));
    PanelTimer timer(&w, S(stream_));
    Check(milp_launch::panel_interleave(width, w.flat.get(), ncols, ncols, kp, w.cols.get(),
                                        S(stream_)),
          "row panel interleave");
    if (sink.ranges) {
      Check(milp_launch::panel_interleave(width, w.flat.get() + up, ncols, ncols, kp,
                                          w.cols_upper.get(), S(stream_)),
            "row panel interleave");
    }
    RowPanelSums(first, kp, width, &timer, sink);
  });
}

// The k points base + overrides: base and the lists go up once, every panel
// is filled and overridden on the device, then RowPanelSums.
int64_t DeviceLp::RowPanelsFrom(const double* base, const double* base_upper, int k,
                                const int64_t* starts, const int32_t* cols, const double* vals,
                                const double* vals_upper, const RowPanelSink& sink) {
  PanelWorkspace& w = *panel_;
  const int ncols = sink.ranges ? n_total_ - m_ : n_total_;
  const int64_t overrides = starts[k];
  Upload(w.base.Reserve(size_t(ncols), "panel base point"), base, size_t(ncols) * sizeof(double));
  Upload(w.ov_starts.Reserve(size_t(k) + 1, "panel override starts"), starts,
         (size_t(k) + 1) * sizeof(int64_t));
  Upload(w.ov_cols.Reserve(size_t(overrides), "panel override columns"), cols,
         size_t(overrides) * sizeof(int32_t));
  Upload(w.ov_vals.Reserve(size_t(overrides), "panel override values"), vals,
         size_t(overrides) * sizeof(double));
  if (sink.ranges) {
    Upload(w.base_upper.Reserve(size_t(ncols), "panel base upper bounds"), base_upper,
           size_t(ncols) * sizeof(double));
    Upload(w.ov_vals_upper.Reserve(size_t(overrides), "panel override upper bounds"), vals_upper,
           size_t(overrides) * sizeof(double));
  }
  // One interleaved array of the panel: the base in every point, then the
  // panel's overrides.
  auto build = [&](const double* device_base, const double* device_vals, double* points,
                   int first, int kp, int width) {
    Check(milp_launch::panel_fill(width, device_base, ncols, kp, points, S(stream_)),
          "row panel fill");
    milp_kernels::RowPanelOverrideArgs o{};
    o.starts = w.ov_starts.get() + first;
    o.cols = w.ov_cols.get();
    o.vals = device_vals;
    o.kp = kp;
    o.x = points;
    Check(milp_launch::panel_override(width, o, starts[first + kp] - starts[first], S(stream_)),
          "row panel overrides");
  };
  ForEachPanel(k, [&](int first, int kp, int width) {
    PanelReserve(width, kp, sink.ranges, sink.implied, sink.propagate != nullptr);
    PanelTimer timer(&w, S(stream_));
    build(w.base.get(), w.ov_vals.get(), w.cols.get(), first, kp, width);
    if (sink.ranges) {
      build(w.base_upper.get(), w.ov_vals_upper.get(), w.cols_upper.get(), first, kp, width);
    }
    RowPanelSums(first, kp, width, &timer, sink);
  });
  const int arrays = sink.ranges ? 2 : 1;
  return 8 * int64_t(ncols) * arrays + (4 + 8 * arrays) * overrides + 8 * (int64_t(k) + 1);
}

void DeviceLp::RowSumsPanel(const double* x, int k, double* out) {
  panel_->last_row_panel = LastRowPanel();
  if (k <= 0 || m_ <= 0) return;
  DeviceOp("row sums panel");
  RowPanelSink sink;
  sink.sums = out;
  RowPanels(x, nullptr, k, sink);
  DeviceOp("row sums panel done");
}

void DeviceLp::RowSumsPanelFrom(const double* base, int k, const int64_t* starts,
                                const int32_t* cols, const double* vals, double* out) {
  panel_->last_row_panel = LastRowPanel();
  if (k <= 0 || m_ <= 0) return;
  DeviceOp("row sums panel from");
  RowPanelSink sink;
  sink.sums = out;
  panel_->last_row_panel.overrides_up_bytes =
      RowPanelsFrom(base, nullptr, k, starts, cols, vals, nullptr, sink);
  DeviceOp("row sums panel from done");
}

static_assert(sizeof(milp_kernels::PointViolations) == sizeof(mi_lp_point_violations) &&
                  sizeof(mi_lp_point_violations) == 24 &&
                  offsetof(milp_kernels::PointViolations, worst) ==
                      offsetof(mi_lp_point_violations, worst) &&
                  offsetof(milp_kernels::PointViolations, worst_row) ==
                      offsetof(mi_lp_point_violations, worst_row),
              "kernel_args.h restates mi_lp_point_violations");

DeviceLp::LastRowViolations DeviceLp::last_row_violations() const {
  return panel_->last_row_violations;
}

// The interleaved sums of one panel are in `rows`: count, offsets, fold and
// write on the device; then down come the kp totals (lists), the kp
// summaries (summaries) and exactly the kept entries, appended point-major.
void DeviceLp::RowPanelViolations(int first, int kp, int width, PanelTimer* timer,
                                  const RowPanelSink& sink) {
  PanelWorkspace& w = *panel_;
  RowViolations* out = sink.violations;
  const int tiles = (m_ + milp_kernels::kPanelTileColumns - 1) / milp_kernels::kPanelTileColumns;
  w.counts.Reserve(size_t(kp) * tiles, "panel counts");
  w.tile_worst.Reserve(size_t(kp) * tiles, "panel tile worst");
  w.tile_worst_row.Reserve(size_t(kp) * tiles, "panel tile worst row");
  milp_kernels::RowViolationArgs a{};
  a.in = w.rows.get();
  a.num_rows = m_;
  a.kp = kp;
  a.tiles = tiles;
  a.row_lb = w.row_lb.get();
  a.row_ub = w.row_ub.get();
  a.tolerance = sink.tolerance;
  a.counts = w.counts.get();
  a.tile_worst = w.tile_worst.get();
  a.tile_worst_row = w.tile_worst_row.get();
  const int64_t* totals = nullptr;
  if (sink.lists) {
    // `flat` held the points on their way up; the interleave that read them
    // is ahead of the write pass on the stream.
    w.kept_cols.Reserve(size_t(m_) * kp, "panel kept rows");
    w.offsets.Reserve(size_t(kp) * tiles + milp_kernels::kPanelMaxWidth, "panel offsets");
    totals = w.totals.Reserve(milp_kernels::kPanelMaxWidth, "panel totals");
    a.offsets = w.offsets.get();
    a.totals = w.offsets.get() + size_t(kp) * tiles;
    a.rows = w.kept_cols.get();
    a.activities = w.flat.get();
  }
  const milp_kernels::PointViolations* host_summaries = nullptr;
  if (sink.summaries) {
    a.summaries = w.summaries.Reserve(milp_kernels::kPanelMaxWidth, "panel summaries");
    host_summaries = w.summaries_host.Reserve(milp_kernels::kPanelMaxWidth, "panel summaries");
  }
  const int rule =
      sink.ranges ? milp_kernels::kRowRuleAboveTolerance : milp_kernels::kRowRuleOutsideBounds;
  Check(milp_launch::row_violations_panel(width, rule, a, S(stream_)), "row violations panel");
  timer->Launched();
  if (sink.summaries) {
    Download(w.summaries_host.get(), a.summaries, size_t(kp) * sizeof(*a.summaries));
    for (int v = 0; v < kp; ++v) {
      const milp_kernels::PointViolations& s = host_summaries[v];
      if (s.count < 0 || s.count > m_ || s.worst_row < -1 || s.worst_row >= m_) {
        throw DeviceError("row violations panel: bad summary");
      }
      mi_lp_point_violations& d = out->summaries[first + v];
      d.count = s.count;
      d.worst = s.worst;
      d.worst_row = s.worst_row;
      d.reserved = 0;
    }
    sink.record->bytes_down += int64_t(kp) * 24;
  }
  int64_t kept = 0;
  if (sink.lists) {
    Download(w.totals.get(), a.totals, size_t(kp) * sizeof(int64_t));
    for (int v = 0; v < kp; ++v) {
      if (totals[v] < 0 || totals[v] > m_) throw DeviceError("row violations panel: bad count");
      kept += totals[v];
      out->row_starts[first + v + 1] = out->row_starts[first + v] + totals[v];
    }
    const size_t old = out->rows.size();
    out->rows.resize(old + size_t(kept));
    out->activities.resize(old + size_t(kept));
    if (kept > 0) {
      Check(hipMemcpyAsync(out->rows.data() + old, a.rows, size_t(kept) * sizeof(int32_t),
                           hipMemcpyDeviceToHost, S(stream_)),
            "D2H");
      Download(out->activities.data() + old, a.activities, size_t(kept) * sizeof(double));
    }
    sink.record->bytes_down += int64_t(kp) * 8 + kept * 12;
  }
  timer->Downloaded();
  sink.record->panels += 1;
  sink.record->width = width;
  sink.record->kept += kept;
}

bool DeviceLp::RowViolationsBegin(LastRowViolations* record, int k, const double* row_lb,
                                  const double* row_ub, bool lists, bool summaries,
                                  RowViolations* out) {
  PanelWorkspace& w = *panel_;
  *record = LastRowViolations();
  record->lists = lists;
  const size_t points = size_t(std::max(k, 0));
  out->row_starts.assign(lists ? points + 1 : 0, 0);
  out->rows.clear();
  out->activities.clear();
  out->summaries.assign(summaries ? points : 0, mi_lp_point_violations{0, 0.0, -1, 0});
  if (k <= 0 || m_ <= 0) return false;
  Upload(w.row_lb.Reserve(size_t(m_), "panel row lower bounds"), row_lb,
         size_t(m_) * sizeof(double));
  Upload(w.row_ub.Reserve(size_t(m_), "panel row upper bounds"), row_ub,
         size_t(m_) * sizeof(double));
  return true;
}

void DeviceLp::RowViolationsPanel(const double* x, int k, const double* row_lb,
                                  const double* row_ub, double tolerance, bool lists,
                                  bool summaries, RowViolations* out) {
  if (!RowViolationsBegin(&panel_->last_row_violations, k, row_lb, row_ub, lists, summaries,
                          out)) {
    return;
  }
  DeviceOp("row violations panel");
  RowPanelSink sink;
  sink.violations = out;
  sink.tolerance = tolerance;
  sink.lists = lists;
  sink.summaries = summaries;
  sink.record = &panel_->last_row_violations;
  RowPanels(x, nullptr, k, sink);
  DeviceOp("row violations panel done");
}

void DeviceLp::RowViolationsPanelFrom(const double* base, int k, const int64_t* starts,
                                      const int32_t* cols, const double* vals,
                                      const double* row_lb, const double* row_ub,
                                      double tolerance, bool lists, bool summaries,
                                      RowViolations* out) {
  if (!RowViolationsBegin(&panel_->last_row_violations, k, row_lb, row_ub, lists, summaries,
                          out)) {
    return;
  }
  DeviceOp("row violations panel from");
  RowPanelSink sink;
  sink.violations = out;
  sink.tolerance = tolerance;
  sink.lists = lists;
  sink.summaries = summaries;
  sink.record = &panel_->last_row_violations;
  panel_->last_row_violations.overrides_up_bytes =
      RowPanelsFrom(base, nullptr, k, starts, cols, vals, nullptr, sink);
  DeviceOp("row violations panel from done");
}

DeviceLp::LastBoundRanges DeviceLp::last_bound_ranges() const {
  return panel_->last_bound_ranges;
}

void DeviceLp::BoundRangesPanel(const double* lbs, const double* ubs, int k,
                                double* min_activity, double* max_activity,
                                int32_t* inf_counts) {
  panel_->last_bound_ranges = LastBoundRanges();
  if (k <= 0 || m_ <= 0) return;
  DeviceOp("bound ranges panel");
  RowPanelSink sink;
  sink.ranges = true;
  sink.sums = min_activity;
  sink.max_activity = max_activity;
  sink.inf_counts = inf_counts;
  RowPanels(lbs, ubs, k, sink);
  DeviceOp("bound ranges panel done");
}

void DeviceLp::BoundRangesPanelFrom(const double* base_lb, const double* base_ub, int k,
                                    const int64_t* starts, const int32_t* cols,
                                    const double* new_lbs, const double* new_ubs,
                                    double* min_activity, double* max_activity,
                                    int32_t* inf_counts) {
  panel_->last_bound_ranges = LastBoundRanges();
  if (k <= 0 || m_ <= 0) return;
  DeviceOp("bound ranges panel from");
  RowPanelSink sink;
  sink.ranges = true;
  sink.sums = min_activity;
  sink.max_activity = max_activity;
  sink.inf_counts = inf_counts;
  panel_->last_bound_ranges.overrides_up_bytes =
      RowPanelsFrom(base_lb, base_ub, k, starts, cols, new_lbs, new_ubs, sink);
  DeviceOp("bound ranges panel from done");
}

void DeviceLp::BoundInfeasiblePanel(const double* lbs, const double* ubs, int k,
                                    const double* row_lb, const double* row_ub,
                                    double tolerance, bool lists, RowViolations* out) {
  if (!RowViolationsBegin(&panel_->last_bound_ranges, k, row_lb, row_ub, lists, true, out)) {
    return;
  }
  DeviceOp("bound infeasible panel");
  RowPanelSink sink;
  sink.ranges = true;
  sink.violations = out;
  sink.tolerance = tolerance;
  sink.lists = lists;
  sink.summaries = true;
  sink.record = &panel_->last_bound_ranges;
  RowPanels(lbs, ubs, k, sink);
  DeviceOp("bound infeasible panel done");
}

void DeviceLp::BoundInfeasiblePanelFrom(const double* base_lb, const double* base_ub, int k,
                                        const int64_t* starts, const int32_t* cols,
                                        const double* new_lbs, const double* new_ubs,
                                        const double* row_lb, const double* row_ub,
                                        double tolerance, bool lists, RowViolations* out) {
  if (!RowViolationsBegin(&panel_->last_bound_ranges, k, row_lb, row_ub, lists, true, out)) {
    return;
  }
  DeviceOp("bound infeasible panel from");
  RowPanelSink sink;
  sink.ranges = true;
  sink.violations = out;
  sink.tolerance = tolerance;
  sink.lists = lists;
  sink.summaries = true;
  sink.record = &panel_->last_bound_ranges;
  panel_->last_bound_ranges.overrides_up_bytes =
      RowPanelsFrom(base_lb, base_ub, k, starts, cols, new_lbs, new_ubs, sink);
  DeviceOp("bound infeasible panel from done");
}

DeviceLp::LastBoundImplied DeviceLp::last_bound_implied() const {
  return panel_->last_bound_implied;
}

// The ranges of one panel (lo, hi, packed counts) are in `rows` and the own
// bounds in `cols` / `cols_upper`: the implied bounds into `implied`; then
// the dense form (vector-major into `flat`, down to sink.sums and
// sink.max_activity) or the filtered form (count, offsets, fold and write
// over the keys, a gather of the two bounds at the kept columns; down come
// the kp summaries and, with lists, the kp totals and exactly the kept
// entries, appended set-major).
void DeviceLp::RowPanelImplied(int first, int kp, int width, PanelTimer* timer,
                               const RowPanelSink& sink) {
  PanelWorkspace& w = *panel_;
  LastBoundImplied& record = w.last_bound_implied;
  const int n = n_total_ - m_;
  const size_t block = size_t(n) * width;
  const size_t down = size_t(kp) * n;
  TightenedColumns* out = sink.tightened;
  milp_kernels::ImpliedBoundsArgs a = PanelImpliedArgs(kp, width);
  a.tolerance = sink.tolerance;
  if (out != nullptr && sink.from_base) {
    a.base_lb = w.base.get();
    a.base_ub = w.base_upper.get();
  }
  a.keys = out != nullptr ? w.implied.get() + 2 * block : nullptr;
  Check(milp_launch::implied_bounds_panel(width, sink.long_columns, a, S(stream_)),
        "implied bounds panel");
  record.panels += 1;
  record.width = width;
  record.columns = sink.long_columns ? kPanelLongColumns : kPanelShortColumns;
  if (out == nullptr) {
    Check(milp_launch::panel_deinterleave(width, a.new_lower, n, kp, w.flat.get(), n, S(stream_)),
          "implied bounds de-interleave");
    Check(milp_launch::panel_deinterleave(width, a.new_upper, n, kp, w.flat.get() + down, n,
                                          S(stream_)),
          "implied bounds de-interleave");
    timer->Launched();
    Check(hipMemcpyAsync(sink.max_activity + size_t(first) * n, w.flat.get() + down,
                         down * sizeof(double), hipMemcpyDeviceToHost, S(stream_)),
          "D2H");
    Download(sink.sums + size_t(first) * n, w.flat.get(), down * sizeof(double));
    timer->Downloaded();
    record.bytes_down += 16 * int64_t(down);
    return;
  }
  PanelKeptColumns(first, kp, width, a.keys, a.new_lower, a.new_upper, sink.lists, timer, out,
                   &record.kept, &record.bytes_down, "tightened columns panel");
}

milp_kernels::ImpliedBoundsArgs DeviceLp::PanelImpliedArgs(int kp, int width) const {
  PanelWorkspace& w = *panel_;
  const int n = n_total_ - m_;
  milp_kernels::ImpliedBoundsArgs a{};
  a.starts = d_starts_;
  a.rows = d_rows_;
  a.vals = d_vals_;
  a.ranges = w.rows.get();
  a.row_lb = w.row_lb.get();
  a.row_ub = w.row_ub.get();
  a.lower = w.cols.get();
  a.upper = w.cols_upper.get();
  a.num_rows = m_;
  a.num_cols = n;
  a.kp = kp;
  a.new_lower = w.implied.get();
  a.new_upper = w.implied.get() + size_t(n) * width;
  return a;
}

void DeviceLp::PanelKeptColumns(int first, int kp, int width, const double* keys,
                                const double* lower, const double* upper, bool lists,
                                PanelTimer* timer, TightenedColumns* out, int64_t* kept_total,
                                int64_t* bytes_down, const char* what) {
  PanelWorkspace& w = *panel_;
  const int n = n_total_ - m_;
  const size_t down = size_t(kp) * n;
  const int tiles = (n + milp_kernels::kPanelTileColumns - 1) / milp_kernels::kPanelTileColumns;
  w.counts.Reserve(size_t(kp) * tiles, "panel counts");
  w.tile_worst.Reserve(size_t(kp) * tiles, "panel tile worst");
  w.tile_worst_row.Reserve(size_t(kp) * tiles, "panel tile worst row");
  milp_kernels::RowViolationArgs v{};
  v.in = keys;
  v.num_rows = n;
  v.kp = kp;
  v.tiles = tiles;
  v.counts = w.counts.get();
  v.tile_worst = w.tile_worst.get();
  v.tile_worst_row = w.tile_worst_row.get();
  const int64_t* totals = nullptr;
  if (lists) {
    w.kept_cols.Reserve(size_t(n) * kp, "panel kept columns");
    w.offsets.Reserve(size_t(kp) * tiles + milp_kernels::kPanelMaxWidth, "panel offsets");
    totals = w.totals.Reserve(milp_kernels::kPanelMaxWidth, "panel totals");
    v.offsets = w.offsets.get();
    v.totals = w.offsets.get() + size_t(kp) * tiles;
    v.rows = w.kept_cols.get();
    v.activities = w.flat.get() + 2 * down;  // the kept keys; not brought down
  }
  v.summaries = w.summaries.Reserve(milp_kernels::kPanelMaxWidth, "panel summaries");
  const milp_kernels::PointViolations* host_summaries =
      w.summaries_host.Reserve(milp_kernels::kPanelMaxWidth, "panel summaries");
  Check(milp_launch::row_violations_panel(width, milp_kernels::kRowRuleKeptKey, v, S(stream_)),
        what);
  if (lists) {
    milp_kernels::ImpliedGatherArgs g{};
    g.totals = v.totals;
    g.cols = v.rows;
    g.new_lower = lower;
    g.new_upper = upper;
    g.num_cols = n;
    g.kp = kp;
    g.out_lower = w.flat.get();
    g.out_upper = w.flat.get() + down;
    Check(milp_launch::implied_gather(width, g, S(stream_)), what);
  }
  timer->Launched();
  Download(w.summaries_host.get(), v.summaries, size_t(kp) * sizeof(*v.summaries));
  for (int c = 0; c < kp; ++c) {
    const milp_kernels::PointViolations& s = host_summaries[c];
    if (s.count < 0 || s.count > n || s.worst_row < -1 || s.worst_row >= n) {
      throw DeviceError(std::string(what) + ": bad summary");
    }
    mi_lp_point_violations& d = out->summaries[first + c];
    d.count = s.count;
    d.worst = s.worst;
    d.worst_row = s.worst_row;
    d.reserved = 0;
  }
  *bytes_down += int64_t(kp) * 24;
  if (lists) {
    Download(w.totals.get(), v.totals, size_t(kp) * sizeof(int64_t));
    int64_t kept = 0;
    for (int c = 0; c < kp; ++c) {
      if (totals[c] < 0 || totals[c] > n) throw DeviceError(std::string(what) + ": bad count");
      kept += totals[c];
      out->col_starts[first + c + 1] = out->col_starts[first + c] + totals[c];
    }
    const size_t old = out->cols.size();
    out->cols.resize(old + size_t(kept));
    out->new_lbs.resize(old + size_t(kept));
    out->new_ubs.resize(old + size_t(kept));
    if (kept > 0) {
      Check(hipMemcpyAsync(out->cols.data() + old, v.rows, size_t(kept) * sizeof(int32_t),
                           hipMemcpyDeviceToHost, S(stream_)),
            "D2H");
      Check(hipMemcpyAsync(out->new_ubs.data() + old, w.flat.get() + down,
                           size_t(kept) * sizeof(double), hipMemcpyDeviceToHost, S(stream_)),
            "D2H");
      Download(out->new_lbs.data() + old, w.flat.get(), size_t(kept) * sizeof(double));
    }
    *kept_total += kept;
    *bytes_down += int64_t(kp) * 8 + kept * 20;
  }
  timer->Downloaded();
}

bool DeviceLp::BoundImpliedBegin(int k, const double* row_lb, const double* row_ub, bool lists,
                                 TightenedColumns* out, RowPanelSink* sink) {
  PanelWorkspace& w = *panel_;
  w.last_bound_implied = LastBoundImplied();
  w.last_bound_implied.lists = lists;
  const size_t sets = size_t(std::max(k, 0));
  if (out != nullptr) {
    out->col_starts.assign(lists ? sets + 1 : 0, 0);
    out->cols.clear();
    out->new_lbs.clear();
    out->new_ubs.clear();
    out->summaries.assign(sets, mi_lp_point_violations{0, 0.0, -1, 0});
  }
  if (!PanelImpliedSetup(k, row_lb, row_ub, sink)) return false;
  w.last_bound_implied.bytes_up = 16 * int64_t(m_);
  sink->tightened = out;
  sink->lists = lists;
  return true;
}

bool DeviceLp::PanelImpliedSetup(int k, const double* row_lb, const double* row_ub,
                                 RowPanelSink* sink) {
  PanelWorkspace& w = *panel_;
  const int n = n_total_ - m_;
  if (k <= 0 || m_ <= 0 || n <= 0) return false;
  Upload(w.row_lb.Reserve(size_t(m_), "panel row lower bounds"), row_lb,
         size_t(m_) * sizeof(double));
  Upload(w.row_ub.Reserve(size_t(m_), "panel row upper bounds"), row_ub,
         size_t(m_) * sizeof(double));
  // Long columns when the structural entries per structural column are >= 32.
  // PanelKernelChoice's average leaves the dense block's columns out.
  bool long_columns = double(h_starts_[n]) / n >= 32.0;
  if (const char* env = std::getenv("MILP_IMPLIED_COLUMNS")) {
    const std::string shape(env);
    if (shape == "short") long_columns = false;
    if (shape == "long") long_columns = true;
  }
  sink->ranges = true;
  sink->implied = true;
  sink->long_columns = long_columns;
  return true;
}

void DeviceLp::BoundImpliedPanel(const double* lbs, const double* ubs, int k,
                                 const double* row_lb, const double* row_ub, double* new_lbs,
                                 double* new_ubs) {
  RowPanelSink sink;
  if (!BoundImpliedBegin(k, row_lb, row_ub, false, nullptr, &sink)) {
    // Without rows or columns to walk, every column keeps its bounds.
    const size_t all = size_t(std::max(k, 0)) * size_t(n_total_ - m_);
    if (all > 0) {
      std::copy(lbs, lbs + all, new_lbs);
      std::copy(ubs, ubs + all, new_ubs);
    }
    return;
  }
  DeviceOp("bound implied panel");
  sink.sums = new_lbs;
  sink.max_activity = new_ubs;
  RowPanels(lbs, ubs, k, sink);
  panel_->last_bound_implied.bytes_up += 16 * int64_t(k) * (n_total_ - m_);
  DeviceOp("bound implied panel done");
}

void DeviceLp::BoundImpliedPanelFrom(const double* base_lb, const double* base_ub, int k,
                                     const int64_t* starts, const int32_t* cols,
                                     const double* ov_lbs, const double* ov_ubs,
                                     const double* row_lb, const double* row_ub, double* new_lbs,
                                     double* new_ubs) {
  RowPanelSink sink;
  if (!BoundImpliedBegin(k, row_lb, row_ub, false, nullptr, &sink)) return;
  DeviceOp("bound implied panel from");
  sink.sums = new_lbs;
  sink.max_activity = new_ubs;
  sink.from_base = true;
  panel_->last_bound_implied.bytes_up +=
      RowPanelsFrom(base_lb, base_ub, k, starts, cols, ov_lbs, ov_ubs, sink);
  DeviceOp("bound implied panel from done");
}

void DeviceLp::BoundTightenedPanel(const double* lbs, const double* ubs, int k,
                                   const double* row_lb, const double* row_ub, double tolerance,
                                   bool lists, TightenedColumns* out) {
  RowPanelSink sink;
  if (!BoundImpliedBegin(k, row_lb, row_ub, lists, out, &sink)) return;
  DeviceOp("bound tightened panel");
  sink.tolerance = tolerance;
  RowPanels(lbs, ubs, k, sink);
  panel_->last_bound_implied.bytes_up += 16 * int64_t(k) * (n_total_ - m_);
  DeviceOp("bound tightened panel done");
}

void DeviceLp::BoundTightenedPanelFrom(const double* base_lb, const double* base_ub, int k,
                                       const int64_t* starts, const int32_t* cols,
                                       const double* ov_lbs, const double* ov_ubs,
                                       const double* row_lb, const double* row_ub,
                                       double tolerance, bool lists, TightenedColumns* out) {
  RowPanelSink sink;
  if (!BoundImpliedBegin(k, row_lb, row_ub, lists, out, &sink)) return;
  DeviceOp("bound tightened panel from");
  sink.tolerance = tolerance;
  sink.from_base = true;
  panel_->last_bound_implied.bytes_up +=
      RowPanelsFrom(base_lb, base_ub, k, starts, cols, ov_lbs, ov_ubs, sink);
  DeviceOp("bound tightened panel from done");
}

DeviceLp::LastBoundPropagate DeviceLp::last_bound_propagate() const {
  return panel_->last_bound_propagate;
}

namespace {
const mi_lp_propagation kPropagationStart = {MI_LP_PROPAGATE_ROUND_LIMIT, 0, 0, 0.0, -1, 0};

bool SameBits(double a, double b) {
  uint64_t x, y;
  std::memcpy(&x, &a, sizeof(x));
  std::memcpy(&y, &b, sizeof(y));
  return x == y;
}

// Columns of (l, u) that differ in bits from (from_l, from_u).
int32_t ChangedColumns(const double* l, const double* u, const double* from_l,
                       const double* from_u, int n) {
  int32_t changed = 0;
  for (int c = 0; c < n; ++c) {
    if (!SameBits(l[c], from_l[c]) || !SameBits(u[c], from_u[c])) ++changed;
  }
  return changed;
}

// Set j of base + overrides into l / u (n each).
void MaterialiseSet(const double* base_lb, const double* base_ub, int n, int j,
                    const int64_t* starts, const int32_t* cols, const double* ov_lbs,
                    const double* ov_ubs, double* l, double* u) {
  std::copy(base_lb, base_lb + n, l);
  std::copy(base_ub, base_ub + n, u);
  for (int64_t i = starts[j]; i < starts[j + 1]; ++i) {
    l[cols[i]] = ov_lbs[i];
    u[cols[i]] = ov_ubs[i];
  }
}
}  // namespace

// The sets of one panel are in `cols` / `cols_upper`. Every round ends with a
// synchronizing download of kp summaries; the timer covers each stretch of
// launches on its own.
void DeviceLp::RowPanelPropagate(int first, int kp, int width, PanelTimer* timer,
                                 const RowPanelSink& sink) {
  PanelWorkspace& w = *panel_;
  LastBoundPropagate& record = w.last_bound_propagate;
  const PropagateParams& params = *sink.propagate;
  const int n = n_total_ - m_;
  const size_t block = size_t(n) * width;
  const size_t down = size_t(kp) * n;
  const int tiles = (n + milp_kernels::kPanelTileColumns - 1) / milp_kernels::kPanelTileColumns;
  w.counts.Reserve(size_t(kp) * tiles, "panel counts");
  w.tile_worst.Reserve(size_t(kp) * tiles, "panel tile worst");
  w.tile_worst_row.Reserve(size_t(kp) * tiles, "panel tile worst row");
  const milp_kernels::ImpliedBoundsArgs implied = PanelImpliedArgs(kp, width);
  milp_kernels::PropagateApplyArgs apply{};
  apply.new_lower = implied.new_lower;
  apply.new_upper = implied.new_upper;
  apply.lower = w.cols.get();
  apply.upper = w.cols_upper.get();
  apply.is_integer = params.is_integer != nullptr ? w.is_integer.get() : nullptr;
  apply.num_cols = n;
  apply.kp = kp;
  apply.tolerance = params.tolerance;
  apply.integrality_tolerance = params.integrality_tolerance;
  apply.keys = w.implied.get() + 2 * block;
  double* const moved_keys = w.implied.get() + 3 * block;
  milp_kernels::RowViolationArgs v{};  // summaries only: count and fold
  v.num_rows = n;
  v.kp = kp;
  v.tiles = tiles;
  v.counts = w.counts.get();
  v.tile_worst = w.tile_worst.get();
  v.tile_worst_row = w.tile_worst_row.get();
  v.summaries = w.summaries.Reserve(milp_kernels::kPanelMaxWidth, "panel summaries");
  const milp_kernels::PointViolations* host_summaries =
      w.summaries_host.Reserve(milp_kernels::kPanelMaxWidth, "panel summaries");
  // The kp summaries of `keys`, down.
  auto summarise = [&](const double* keys) {
    v.in = keys;
    Check(milp_launch::row_violations_panel(width, milp_kernels::kRowRuleKeptKey, v, S(stream_)),
          "bound propagate summaries");
    timer->Launched();
    Download(w.summaries_host.get(), v.summaries, size_t(kp) * sizeof(*v.summaries));
    timer->Downloaded();
    for (int c = 0; c < kp; ++c) {
      const milp_kernels::PointViolations& s = host_summaries[c];
      if (s.count < 0 || s.count > n || s.worst_row < -1 || s.worst_row >= n) {
        throw DeviceError("bound propagate panel: bad summary");
      }
    }
    record.bytes_down += int64_t(kp) * 24;
    timer->Restart();
  };
  mi_lp_propagation* out = sink.propagation + first;
  const uint32_t all = (uint32_t{1} << kp) - 1;  // kp <= kPanelMaxWidth = 16
  uint32_t stopped = 0;
  for (int round = 1; round <= params.max_rounds && stopped != all; ++round) {
    PanelLaunchRanges(kp, width, false);
    Check(milp_launch::implied_bounds_panel(width, sink.long_columns, implied, S(stream_)),
          "implied bounds panel");
    apply.frozen = stopped;
    apply.moved_keys = round == 1 ? moved_keys : nullptr;
    Check(milp_launch::propagate_apply(width, apply, S(stream_)), "bound propagate apply");
    summarise(apply.keys);
    record.rounds += 1;
    uint32_t recount = 0;  // stopped INFEASIBLE in round 1: own bounds may cross without a move
    for (int c = 0; c < kp; ++c) {
      if ((stopped >> c) & 1u) continue;
      const milp_kernels::PointViolations& s = host_summaries[c];
      out[c].rounds = round;
      if (s.worst_row >= 0) {
        out[c].status = MI_LP_PROPAGATE_INFEASIBLE;
        out[c].worst = s.worst;
        out[c].worst_col = s.worst_row;
        stopped |= uint32_t{1} << c;
        if (round == 1) {
          recount |= uint32_t{1} << c;
        } else {
          out[c].moves += s.count;
        }
      } else if (s.count == 0) {
        out[c].status = MI_LP_PROPAGATE_FIXPOINT;
        stopped |= uint32_t{1} << c;
      } else {
        out[c].moves += s.count;
      }
    }
    if (recount != 0) {
      summarise(moved_keys);
      for (int c = 0; c < kp; ++c) {
        if ((recount >> c) & 1u) out[c].moves += host_summaries[c].count;
      }
    }
  }
  record.panels += 1;
  record.width = width;
  record.columns = sink.long_columns ? kPanelLongColumns : kPanelShortColumns;
  if (sink.tightened == nullptr) {
    Check(milp_launch::panel_deinterleave(width, w.cols.get(), n, kp, w.flat.get(), n, S(stream_)),
          "bound propagate de-interleave");
    Check(milp_launch::panel_deinterleave(width, w.cols_upper.get(), n, kp, w.flat.get() + down, n,
                                          S(stream_)),
          "bound propagate de-interleave");
    timer->Launched();
    Check(hipMemcpyAsync(sink.final_ubs + size_t(first) * n, w.flat.get() + down,
                         down * sizeof(double), hipMemcpyDeviceToHost, S(stream_)),
          "D2H");
    Download(sink.final_lbs + size_t(first) * n, w.flat.get(), down * sizeof(double));
    timer->Downloaded();
    record.bytes_down += 16 * int64_t(down);
    return;
  }
  milp_kernels::PropagateChangedArgs changed{};
  changed.lower = w.cols.get();
  changed.upper = w.cols_upper.get();
  changed.base_lb = w.base.get();
  changed.base_ub = w.base_upper.get();
  changed.num_cols = n;
  changed.kp = kp;
  changed.tolerance = params.tolerance;
  changed.keys = apply.keys;
  Check(milp_launch::propagate_changed_keys(width, changed, S(stream_)),
        "bound propagate changed keys");
  PanelKeptColumns(first, kp, width, changed.keys, changed.lower, changed.upper, sink.lists, timer,
                   sink.tightened, &record.kept, &record.bytes_down, "bound propagated columns");
  for (int c = 0; c < kp; ++c) {
    out[c].kept = static_cast<int32_t>(sink.tightened->summaries[first + c].count);
  }
}

void DeviceLp::PropagateWithoutRows(const PropagateParams& params, int n, double* l, double* u,
                                    mi_lp_propagation* summary) {
  *summary = kPropagationStart;
  for (int round = 1; round <= params.max_rounds; ++round) {
    int64_t moves = 0;
    double worst = 0.0;
    int worst_col = -1;
    for (int c = 0; c < n; ++c) {  // without rows the implied bounds are the own ones
      double nl = l[c];
      double nu = u[c];
      if (params.is_integer != nullptr && params.is_integer[c] != 0) {
        nl = std::ceil(nl - params.integrality_tolerance) + 0.0;
        nu = std::floor(nu + params.integrality_tolerance) + 0.0;
      }
      if ((nl - l[c] > params.tolerance) || (u[c] - nu > params.tolerance)) {
        l[c] = nl;
        u[c] = nu;
        ++moves;
      }
      const double cross = l[c] - u[c];
      if (cross > params.tolerance && cross > worst) {
        worst = cross;
        worst_col = c;
      }
    }
    summary->rounds = round;
    summary->moves += moves;
    if (worst_col >= 0) {
      summary->status = MI_LP_PROPAGATE_INFEASIBLE;
      summary->worst = worst;
      summary->worst_col = worst_col;
      return;
    }
    if (moves == 0) {
      summary->status = MI_LP_PROPAGATE_FIXPOINT;
      return;
    }
  }
}

bool DeviceLp::BoundPropagateBegin(int k, const PropagateParams& params, const double* row_lb,
                                   const double* row_ub, bool lists, PropagatedColumns* out,
                                   mi_lp_propagation* summaries, RowPanelSink* sink) {
  PanelWorkspace& w = *panel_;
  w.last_bound_propagate = LastBoundPropagate();
  w.last_bound_propagate.lists = lists;
  const size_t sets = size_t(std::max(k, 0));
  if (out != nullptr) {
    out->lists.col_starts.assign(lists ? sets + 1 : 0, 0);
    out->lists.cols.clear();
    out->lists.new_lbs.clear();
    out->lists.new_ubs.clear();
    out->lists.summaries.assign(sets, mi_lp_point_violations{0, 0.0, -1, 0});
    out->summaries.assign(sets, kPropagationStart);
    summaries = out->summaries.data();
  } else {
    std::fill(summaries, summaries + sets, kPropagationStart);
  }
  if (!PanelImpliedSetup(k, row_lb, row_ub, sink)) return false;
  const int n = n_total_ - m_;
  w.last_bound_propagate.bytes_up = 16 * int64_t(m_);
  if (params.is_integer != nullptr) {
    Upload(w.is_integer.Reserve(size_t(n), "panel integer columns"), params.is_integer, size_t(n));
    w.last_bound_propagate.bytes_up += n;
  }
  sink->propagate = &params;
  sink->propagation = summaries;
  sink->tolerance = params.tolerance;
  sink->tightened = out != nullptr ? &out->lists : nullptr;
  sink->lists = lists;
  return true;
}

void DeviceLp::BoundPropagatePanel(const double* lbs, const double* ubs, int k,
                                   const PropagateParams& params, const double* row_lb,
                                   const double* row_ub, double* new_lbs, double* new_ubs,
                                   mi_lp_propagation* summaries) {
  const int n = n_total_ - m_;
  RowPanelSink sink;
  if (BoundPropagateBegin(k, params, row_lb, row_ub, false, nullptr, summaries, &sink)) {
    DeviceOp("bound propagate panel");
    sink.final_lbs = new_lbs;
    sink.final_ubs = new_ubs;
    RowPanels(lbs, ubs, k, sink);
    panel_->last_bound_propagate.bytes_up += 16 * int64_t(k) * n;
    DeviceOp("bound propagate panel done");
  } else {
    for (int j = 0; j < k; ++j) {
      std::copy(lbs + size_t(j) * n, lbs + size_t(j + 1) * n, new_lbs + size_t(j) * n);
      std::copy(ubs + size_t(j) * n, ubs + size_t(j + 1) * n, new_ubs + size_t(j) * n);
      PropagateWithoutRows(params, n, new_lbs + size_t(j) * n, new_ubs + size_t(j) * n,
                           &summaries[j]);
    }
  }
  for (int j = 0; j < k; ++j) {
    const size_t at = size_t(j) * n;
    summaries[j].kept = ChangedColumns(new_lbs + at, new_ubs + at, lbs + at, ubs + at, n);
  }
}

void DeviceLp::BoundPropagatePanelFrom(const double* base_lb, const double* base_ub, int k,
                                       const int64_t* starts, const int32_t* cols,
                                       const double* ov_lbs, const double* ov_ubs,
                                       const PropagateParams& params, const double* row_lb,
                                       const double* row_ub, double* new_lbs, double* new_ubs,
                                       mi_lp_propagation* summaries) {
  const int n = n_total_ - m_;
  RowPanelSink sink;
  const bool launch =
      BoundPropagateBegin(k, params, row_lb, row_ub, false, nullptr, summaries, &sink);
  if (launch) {
    DeviceOp("bound propagate panel from");
    sink.final_lbs = new_lbs;
    sink.final_ubs = new_ubs;
    sink.from_base = true;
    panel_->last_bound_propagate.bytes_up +=
        RowPanelsFrom(base_lb, base_ub, k, starts, cols, ov_lbs, ov_ubs, sink);
    DeviceOp("bound propagate panel from done");
  }
  std::vector<double> l(size_t(std::max(n, 0))), u(size_t(std::max(n, 0)));
  for (int j = 0; j < k; ++j) {
    const size_t at = size_t(j) * n;
    MaterialiseSet(base_lb, base_ub, n, j, starts, cols, ov_lbs, ov_ubs, l.data(), u.data());
    if (!launch) {
      std::copy(l.begin(), l.end(), new_lbs + at);
      std::copy(u.begin(), u.end(), new_ubs + at);
      PropagateWithoutRows(params, n, new_lbs + at, new_ubs + at, &summaries[j]);
    }
    summaries[j].kept = ChangedColumns(new_lbs + at, new_ubs + at, l.data(), u.data(), n);
  }
}

void DeviceLp::BoundPropagatedColumnsFrom(const double* base_lb, const double* base_ub, int k,
                                          const int64_t* starts, const int32_t* cols,
                                          const double* ov_lbs, const double* ov_ubs,
                                          const PropagateParams& params, const double* row_lb,
                                          const double* row_ub, bool lists,
                                          PropagatedColumns* out) {
  RowPanelSink sink;
  if (BoundPropagateBegin(k, params, row_lb, row_ub, lists, out, nullptr, &sink)) {
    DeviceOp("bound propagated columns from");
    sink.from_base = true;
    panel_->last_bound_propagate.bytes_up +=
        RowPanelsFrom(base_lb, base_ub, k, starts, cols, ov_lbs, ov_ubs, sink);
    DeviceOp("bound propagated columns from done");
    return;
  }
  // Without rows: the rule and the keep rule on the host.
  const int n = n_total_ - m_;
  std::vector<double> l(size_t(std::max(n, 0))), u(size_t(std::max(n, 0)));
  for (int j = 0; j < k; ++j) {
    MaterialiseSet(base_lb, base_ub, n, j, starts, cols, ov_lbs, ov_ubs, l.data(), u.data());
    PropagateWithoutRows(params, n, l.data(), u.data(), &out->summaries[j]);
    int32_t kept = 0;
    for (int c = 0; c < n; ++c) {
      if (!(l[c] - u[c] > params.tolerance) && SameBits(l[c], base_lb[c]) &&
          SameBits(u[c], base_ub[c])) {
        continue;
      }
      ++kept;
      if (!lists) continue;
      out->lists.cols.push_back(c);
      out->lists.new_lbs.push_back(l[c]);
      out->lists.new_ubs.push_back(u[c]);
    }
    out->summaries[j].kept = kept;
    if (lists) out->lists.col_starts[j + 1] = out->lists.col_starts[j] + kept;
  }
}

}  // namespace milp
