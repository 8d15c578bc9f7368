// TEST SUPPORT ONLY (include/mi_lp_devop.h): one thin call per public
// DeviceLp method, so that a test can run a single device operation on inputs
// it chooses. A handle owns its CompactSparseMatrix pair and its DeviceLp;
// there is no RevisedSimplex behind it.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "../../../include/mi_lp_devop.h"
#include "device_lp.h"
#include "lp_data.h"
#include "lu.h"

struct mi_devop {
  milp::CompactSparseMatrix csc;  // [A | I]
  milp::CompactSparseMatrix csr;  // its transpose
  milp::DeviceLp dev;
  std::vector<uint64_t> relevant;  // the last kRelevant mask
  milp::TriangularMatrix tri;      // tri_set_matrix
  std::string error;
};

namespace {

thread_local std::string g_create_error;

// Runs fn; a DeviceError (or any other exception) becomes a non-zero return
// and the handle's message.
template <typename Fn>
int Guard(mi_devop* h, Fn fn) {
  try {
    fn();
    return 0;
  } catch (const std::exception& e) {
    h->error = e.what();
  } catch (...) {
    h->error = "unknown exception";
  }
  return 1;
}

mi_devop* Create(int device, int m, int n, const int64_t* col_starts, const int32_t* row_idx,
                 const double* vals) {
  mi_devop* h = nullptr;
  try {
    h = new mi_devop();
    h->csc.PopulateFromSparseMatrixAndAddSlacks(m, n, col_starts, row_idx, vals);
    h->csr.PopulateFromTranspose(h->csc);
    h->dev.Init(device);
    h->dev.UploadMatrix(h->csc, h->csr);
    h->relevant.assign((h->csc.num_cols() + 63) / 64, ~0ull);
    return h;
  } catch (const std::exception& e) {
    g_create_error = e.what();
  } catch (...) {
    g_create_error = "unknown exception";
  }
  try {
    delete h;
  } catch (...) {
  }
  return nullptr;
}

void Destroy(mi_devop* h) {
  try {
    delete h;
  } catch (...) {
  }
}

const char* LastError(const mi_devop* h) {
  return h != nullptr ? h->error.c_str() : g_create_error.c_str();
}

int SetMask(mi_devop* h, int which, const uint64_t* words, int num_words) {
  return Guard(h, [&] {
    if (which < 0 || which >= milp::DeviceLp::kNumMasks) throw milp::DeviceError("bad mask");
    h->dev.SetMask(static_cast<milp::DeviceLp::Mask>(which), words, num_words);
    if (which == milp::DeviceLp::kRelevant) h->relevant.assign(words, words + num_words);
  });
}

int SetListMirror(mi_devop* h, int on) {
  return Guard(h, [&] { h->dev.SetListMirror(on != 0); });
}

int SetSmallBatch(mi_devop* h, int on) {
  return Guard(h, [&] { h->dev.SetSmallBatch(on != 0); });
}

int UpdateRowRowWise(mi_devop* h, const int32_t* rows, int k, const double* rho, int algorithm,
                     double drop) {
  return Guard(h, [&] {
    const std::vector<int> filtered(rows, rows + k);
    const std::vector<double> r(rho, rho + h->csc.num_rows());
    h->dev.UpdateRowRowWise(filtered, r, algorithm, drop);
  });
}

int UpdateRowColumnWise(mi_devop* h, const double* rho, double drop, const double* w) {
  return Guard(h, [&] {
    const int m = h->csc.num_rows();
    const std::vector<double> r(rho, rho + m);
    int64_t relevant_entries = 0;
    for (int c = 0; c < h->csc.num_cols(); ++c) {
      if (h->relevant[c >> 6] >> (c & 63) & 1) relevant_entries += h->csc.ColumnNumEntries(c);
    }
    if (w != nullptr) {
      const std::vector<double> wv(w, w + m);
      h->dev.UpdateRowColumnWise(r, drop, relevant_entries, &wv);
    } else {
      h->dev.UpdateRowColumnWise(r, drop, relevant_entries);
    }
  });
}

int FetchUpdateRow(mi_devop* h, int32_t* positions, double* values, int* count) {
  return Guard(h, [&] {
    std::vector<int> p;
    std::vector<double> v;
    h->dev.FetchUpdateRow(&p, &v);
    *count = static_cast<int>(p.size());
    if (!p.empty()) {
      std::memcpy(positions, p.data(), p.size() * sizeof(int32_t));
      std::memcpy(values, v.data(), v.size() * sizeof(double));
    }
  });
}

int ReadCoefficient(mi_devop* h, int col, double* out) {
  return Guard(h, [&] { *out = h->dev.ReadCoefficient(col); });
}

int DownloadCoefficients(mi_devop* h, double* out) {
  return Guard(h, [&] {
    std::vector<double> v;
    h->dev.DownloadCoefficients(&v);
    if (!v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(double));
  });
}

int ListDotsOverUpdateRow(mi_devop* h, const double* v, double* out, int* count) {
  return Guard(h, [&] {
    const std::vector<double> vv(v, v + h->csc.num_rows());
    std::vector<double> o;
    h->dev.ListDotsOverUpdateRow(vv, &o);
    *count = static_cast<int>(o.size());
    if (!o.empty()) std::memcpy(out, o.data(), o.size() * sizeof(double));
  });
}

int ListDots(mi_devop* h, const int32_t* cols, int n, const double* v, double* out) {
  return Guard(h, [&] {
    const std::vector<int> c(cols, cols + n);
    const std::vector<double> vv(v, v + h->csc.num_rows());
    std::vector<double> o;
    h->dev.ListDots(c, vv, &o);
    if (!o.empty()) std::memcpy(out, o.data(), o.size() * sizeof(double));
  });
}

int DualBegin(mi_devop* h, const double* rc, const uint8_t* colbits, const double* bound_diff) {
  return Guard(h, [&] {
    const int n = h->csc.num_cols();
    h->dev.DualBegin(std::vector<double>(rc, rc + n), std::vector<uint8_t>(colbits, colbits + n),
                     std::vector<double>(bound_diff, bound_diff + n));
  });
}

int DualSetColBits(mi_devop* h, const int32_t* cols, const uint8_t* bits, int n) {
  return Guard(h, [&] {
    h->dev.DualSetColBits(std::vector<int32_t>(cols, cols + n),
                          std::vector<uint8_t>(bits, bits + n));
  });
}

int DualRatioCandidates(mi_devop* h, double sign, double threshold, double harris_tolerance,
                        double minimum_delta, double variation_magnitude, int32_t* col,
                        double* coeff, double* rc, int* count, int* list_count) {
  return Guard(h, [&] {
    milp::DeviceLp::DualCandidates c;
    h->dev.DualRatioCandidates(sign, threshold, harris_tolerance, minimum_delta,
                               variation_magnitude, &c);
    *count = static_cast<int>(c.col.size());
    *list_count = c.list_count;
    if (!c.col.empty()) {
      std::memcpy(col, c.col.data(), c.col.size() * sizeof(int32_t));
      std::memcpy(coeff, c.coeff.data(), c.coeff.size() * sizeof(double));
      std::memcpy(rc, c.rc.data(), c.rc.size() * sizeof(double));
    }
  });
}

int DualUpdateReducedCosts(mi_devop* h, double mult, int leaving_col, double leaving_value,
                           int entering_col) {
  return Guard(h, [&] {
    h->dev.DualUpdateReducedCosts(mult, leaving_col, leaving_value, entering_col);
  });
}

int DualDownloadReducedCosts(mi_devop* h, double* rc) {
  return Guard(h, [&] {
    std::vector<double> v;
    h->dev.DualDownloadReducedCosts(&v);
    if (!v.empty()) std::memcpy(rc, v.data(), v.size() * sizeof(double));
  });
}

int LastPaths(mi_devop* h, mi_devop_paths* out) {
  return Guard(h, [&] {
    const milp::DeviceLp::LastPaths p = h->dev.last_paths();
    out->update_row = p.update_row;
    out->compact = p.compact;
    out->ratio = p.ratio;
    out->ratio_tightened = p.ratio_tightened ? 1 : 0;
    out->list_mapped = p.list_mapped ? 1 : 0;
  });
}

int ColumnDotsPanel(mi_devop* h, const double* y, int k, double* out) {
  return Guard(h, [&] { h->dev.ColumnDotsPanel(y, k, out); });
}

int LastPanel(mi_devop* h, mi_devop_panel* out) {
  return Guard(h, [&] {
    const milp::DeviceLp::LastPanel p = h->dev.last_panel();
    out->sparse = p.sparse;
    out->dense = p.dense ? 1 : 0;
    out->panels = p.panels;
    out->width = p.width;
  });
}

int TakeKernelMs(mi_devop* h, double* panel_ms, double* list_dots_ms) {
  return Guard(h, [&] {
    *panel_ms = h->dev.TakePanelKernelMs();
    *list_dots_ms = h->dev.stats().device_ms[MI_K_PRIMAL_NORMS];
    h->dev.ResetStats();
    h->dev.SetTiming(true, 1u << MI_K_PRIMAL_NORMS);
  });
}

int ColumnDotsPanelSparse(mi_devop* h, const double* y, int k, double drop_tolerance,
                          const uint64_t* keep_mask_words, int64_t* row_starts, int32_t* cols,
                          double* vals, int64_t capacity) {
  bool too_large = false;
  const int rc = Guard(h, [&] {
    milp::DeviceLp::SparseRows rows;
    h->dev.ColumnDotsPanelSparse(y, k, drop_tolerance, keep_mask_words, &rows);
    const int64_t kept = rows.row_starts.back();
    if (kept > capacity) {
      too_large = true;
      throw milp::DeviceError("column_dots_panel_sparse: " + std::to_string(kept) +
                              " entries, capacity " + std::to_string(capacity));
    }
    std::memcpy(row_starts, rows.row_starts.data(), rows.row_starts.size() * sizeof(int64_t));
    if (kept > 0) {
      std::memcpy(cols, rows.cols.data(), size_t(kept) * sizeof(int32_t));
      std::memcpy(vals, rows.vals.data(), size_t(kept) * sizeof(double));
    }
  });
  return too_large ? int{MI_DEVOP_CAPACITY} : rc;
}

int LastPanelSparse(mi_devop* h, mi_devop_panel_sparse* out) {
  return Guard(h, [&] {
    const milp::DeviceLp::LastPanelSparse p = h->dev.last_panel_sparse();
    out->sparse = p.panel.sparse;
    out->dense = p.panel.dense ? 1 : 0;
    out->panels = p.panel.panels;
    out->width = p.panel.width;
    out->kept = p.kept;
    out->bytes_down = p.bytes_down;
  });
}

int PanelSparseGeometry(mi_devop_panel_sparse_geometry* out) {
  out->tile_columns = milp::DeviceLp::PanelTileColumns();
  out->offsets_step_tiles = milp::DeviceLp::PanelOffsetsStepTiles();
  return 0;
}

int Pricing(mi_devop* h, const double* c, const double* y, const double* w, double* rc_out,
            double* list_dots_out, int* list_count) {
  return Guard(h, [&] {
    const int m = h->csc.num_rows();
    const int n = h->csc.num_cols();
    const std::vector<double> cv(c, c + n);
    const std::vector<double> yv(y, y + m);
    std::vector<double> rc, dots;
    *list_count = 0;
    if (w != nullptr) {
      const std::vector<double> wv(w, w + m);
      h->dev.Pricing(cv, yv, &rc, &wv, &dots);
      *list_count = static_cast<int>(dots.size());
      if (!dots.empty()) std::memcpy(list_dots_out, dots.data(), dots.size() * sizeof(double));
    } else {
      h->dev.Pricing(cv, yv, &rc);
    }
    if (!rc.empty()) std::memcpy(rc_out, rc.data(), rc.size() * sizeof(double));
  });
}

int ColumnSquaredNorms(mi_devop* h, double* out) {
  return Guard(h, [&] {
    std::vector<double> v;
    h->dev.ColumnSquaredNorms(&v);
    if (!v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(double));
  });
}

int RowSums(mi_devop* h, const double* x, int skip_basic, double sign, double* out) {
  return Guard(h, [&] {
    const std::vector<double> xv(x, x + h->csc.num_cols());
    std::vector<double> v;
    h->dev.RowSums(xv, skip_basic != 0, sign, &v);
    if (!v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(double));
  });
}

int DualBoxedFlips(mi_devop* h, const int32_t* cols, int n, double threshold,
                   uint8_t* flags_out) {
  return Guard(h, [&] {
    std::vector<uint8_t> flags;
    if (cols != nullptr) {
      const std::vector<int> c(cols, cols + n);
      h->dev.DualBoxedFlips(&c, threshold, &flags);
    } else {
      h->dev.DualBoxedFlips(nullptr, threshold, &flags);
    }
    if (!flags.empty()) std::memcpy(flags_out, flags.data(), flags.size());
  });
}

int DualBoxedFlipsEarly(mi_devop* h, const int32_t* cols, int n, double threshold) {
  return Guard(h, [&] {
    h->dev.DualBoxedFlipsEarly(std::vector<int>(cols, cols + n), threshold);
  });
}

int DualTakePricedReducedCosts(mi_devop* h) {
  return Guard(h, [&] { h->dev.DualTakePricedReducedCosts(); });
}

int DualSetReducedCost(mi_devop* h, int col, double value) {
  return Guard(h, [&] { h->dev.DualSetReducedCost(col, value); });
}

int LastColumnDots(mi_devop* h, mi_devop_column_dots* out) {
  return Guard(h, [&] {
    const milp::DeviceLp::LastColumnDots p = h->dev.last_column_dots();
    out->mode = p.mode;
    out->wave_per_col = p.wave_per_col ? 1 : 0;
    out->dense = p.dense ? 1 : 0;
    out->dense_unroll = p.dense_unroll;
  });
}

int LastFlips(mi_devop* h, mi_devop_flips* out) {
  return Guard(h, [&] { out->early_taken = h->dev.last_flips().early_taken ? 1 : 0; });
}

int RowSumsPanel(mi_devop* h, const double* x, int k, double* out) {
  return Guard(h, [&] { h->dev.RowSumsPanel(x, k, out); });
}

int RowSumsPanelFrom(mi_devop* h, const double* base, int k, const int64_t* starts,
                     const int32_t* cols, const double* vals, double* out) {
  return Guard(h, [&] {
    if (!milp::DeviceLp::ValidOverrides(h->csc.num_cols(), k, starts, cols) ||
        (starts[k] > 0 && vals == nullptr)) {
      throw milp::DeviceError("row_sums_panel_from: bad overrides");
    }
    h->dev.RowSumsPanelFrom(base, k, starts, cols, vals, out);
  });
}

int LastRowPanel(mi_devop* h, mi_devop_row_panel* out) {
  return Guard(h, [&] {
    const milp::DeviceLp::LastRowPanel p = h->dev.last_row_panel();
    out->panels = p.panels;
    out->width = p.width;
    out->kernel = p.kernel;
    out->reserved = 0;
    out->overrides_up_bytes = p.overrides_up_bytes;
  });
}

int RowPanelGeometry(mi_devop_row_panel_geometry* out) {
  milp::DeviceLp::RowPanelGeometry(out->rows_per_workgroup, &out->chunk);
  return 0;
}

// The violations and the screening entries: run(lists, summaries, &result),
// then the outputs, unless the lists need more than `capacity` entries.
// any_bounds: +-inf is allowed on either side (the screening).
template <typename Run>
int RowViolationsCall(mi_devop* h, const char* name, bool any_bounds, int k, const double* row_lb,
                      const double* row_ub, double tolerance, int64_t* row_starts, int32_t* rows,
                      double* activities, int64_t capacity, mi_devop_point_violations* summaries,
                      Run run) {
  bool too_large = false;
  const int rc = Guard(h, [&] {
    const int m = h->csc.num_rows();
    bool ok = row_lb != nullptr && row_ub != nullptr && tolerance >= 0.0 &&
              !std::isinf(tolerance) && (row_starts != nullptr || summaries != nullptr);
    for (int r = 0; ok && r < m; ++r) {
      ok = row_lb[r] == row_lb[r] && row_ub[r] == row_ub[r] &&
           (any_bounds || (row_lb[r] < HUGE_VAL && row_ub[r] > -HUGE_VAL));
    }
    if (!ok) throw milp::DeviceError(std::string(name) + ": bad bounds, tolerance or outputs");
    milp::DeviceLp::RowViolations result;
    run(row_starts != nullptr, summaries != nullptr, &result);
    if (row_starts != nullptr) {
      const int64_t kept = result.row_starts.back();
      if (kept > capacity) {
        too_large = true;
        throw milp::DeviceError(std::string(name) + ": " + std::to_string(kept) +
                                " entries, capacity " + std::to_string(capacity));
      }
      std::memcpy(row_starts, result.row_starts.data(),
                  result.row_starts.size() * sizeof(int64_t));
      if (kept > 0) {
        std::memcpy(rows, result.rows.data(), size_t(kept) * sizeof(int32_t));
        std::memcpy(activities, result.activities.data(), size_t(kept) * sizeof(double));
      }
    }
    if (summaries != nullptr && k > 0) {
      std::memcpy(summaries, result.summaries.data(), size_t(k) * sizeof(*summaries));
    }
  });
  return too_large ? int{MI_DEVOP_CAPACITY} : rc;
}

int RowViolationsPanel(mi_devop* h, const double* x, int k, const double* row_lb,
                       const double* row_ub, double tolerance, int64_t* row_starts, int32_t* rows,
                       double* activities, int64_t capacity,
                       mi_devop_point_violations* summaries) {
  return RowViolationsCall(
      h, "row_violations_panel", false, k, row_lb, row_ub, tolerance, row_starts, rows, activities,
      capacity, summaries, [&](bool lists, bool sums, milp::DeviceLp::RowViolations* out) {
        h->dev.RowViolationsPanel(x, k, row_lb, row_ub, tolerance, lists, sums, out);
      });
}

int RowViolationsPanelFrom(mi_devop* h, const double* base, int k, const int64_t* starts,
                           const int32_t* cols, const double* vals, const double* row_lb,
                           const double* row_ub, double tolerance, int64_t* row_starts,
                           int32_t* rows, double* activities, int64_t capacity,
                           mi_devop_point_violations* summaries) {
  return RowViolationsCall(
      h, "row_violations_panel_from", false, k, row_lb, row_ub, tolerance, row_starts, rows,
      activities, capacity, summaries, [&](bool lists, bool sums, milp::DeviceLp::RowViolations* out) {
        if (!milp::DeviceLp::ValidOverrides(h->csc.num_cols(), k, starts, cols) ||
            (starts[k] > 0 && vals == nullptr)) {
          throw milp::DeviceError("row_violations_panel_from: bad overrides");
        }
        h->dev.RowViolationsPanelFrom(base, k, starts, cols, vals, row_lb, row_ub, tolerance,
                                      lists, sums, out);
      });
}

int LastRowViolations(mi_devop* h, mi_devop_row_violations* out) {
  return Guard(h, [&] {
    const milp::DeviceLp::LastRowViolations p = h->dev.last_row_violations();
    out->panels = p.panels;
    out->width = p.width;
    out->lists = p.lists ? 1 : 0;
    out->reserved = 0;
    out->kept = p.kept;
    out->bytes_down = p.bytes_down;
    out->overrides_up_bytes = p.overrides_up_bytes;
  });
}

// The structural columns of the handle's matrix: the bound sets' columns.
int Structural(const mi_devop* h) { return h->csc.num_cols() - h->csc.num_rows(); }

void CheckBoundOverrides(const mi_devop* h, const char* name, int k, const int64_t* starts,
                         const int32_t* cols, const double* new_lbs, const double* new_ubs) {
  if (!milp::DeviceLp::ValidOverrides(Structural(h), k, starts, cols) ||
      (starts[k] > 0 && (new_lbs == nullptr || new_ubs == nullptr))) {
    throw milp::DeviceError(std::string(name) + ": bad overrides");
  }
}

int BoundRangesPanel(mi_devop* h, const double* lbs, const double* ubs, int k,
                     double* min_activity, double* max_activity, int32_t* inf_counts) {
  return Guard(h, [&] {
    h->dev.BoundRangesPanel(lbs, ubs, k, min_activity, max_activity, inf_counts);
  });
}

int BoundRangesPanelFrom(mi_devop* h, const double* base_lb, const double* base_ub, int k,
                         const int64_t* starts, const int32_t* cols, const double* new_lbs,
                         const double* new_ubs, double* min_activity, double* max_activity,
                         int32_t* inf_counts) {
  return Guard(h, [&] {
    CheckBoundOverrides(h, "bound_ranges_panel_from", k, starts, cols, new_lbs, new_ubs);
    h->dev.BoundRangesPanelFrom(base_lb, base_ub, k, starts, cols, new_lbs, new_ubs, min_activity,
                                max_activity, inf_counts);
  });
}

int BoundInfeasiblePanel(mi_devop* h, const double* lbs, const double* ubs, int k,
                         const double* row_lb, const double* row_ub, double tolerance,
                         int64_t* row_starts, int32_t* rows, double* amounts, int64_t capacity,
                         mi_devop_point_violations* summaries) {
  return RowViolationsCall(
      h, "bound_infeasible_panel", true, k, row_lb, row_ub, tolerance, row_starts, rows, amounts,
      capacity, summaries, [&](bool lists, bool, milp::DeviceLp::RowViolations* out) {
        h->dev.BoundInfeasiblePanel(lbs, ubs, k, row_lb, row_ub, tolerance, lists, out);
      });
}

int BoundInfeasiblePanelFrom(mi_devop* h, const double* base_lb, const double* base_ub, int k,
                             const int64_t* starts, const int32_t* cols, const double* new_lbs,
                             const double* new_ubs, const double* row_lb, const double* row_ub,
                             double tolerance, int64_t* row_starts, int32_t* rows,
                             double* amounts, int64_t capacity,
                             mi_devop_point_violations* summaries) {
  return RowViolationsCall(
      h, "bound_infeasible_panel_from", true, k, row_lb, row_ub, tolerance, row_starts, rows,
      amounts, capacity, summaries, [&](bool lists, bool, milp::DeviceLp::RowViolations* out) {
        CheckBoundOverrides(h, "bound_infeasible_panel_from", k, starts, cols, new_lbs, new_ubs);
        h->dev.BoundInfeasiblePanelFrom(base_lb, base_ub, k, starts, cols, new_lbs, new_ubs,
                                        row_lb, row_ub, tolerance, lists, out);
      });
}

int LastBoundRanges(mi_devop* h, mi_devop_row_violations* out) {
  return Guard(h, [&] {
    const milp::DeviceLp::LastBoundRanges p = h->dev.last_bound_ranges();
    out->panels = p.panels;
    out->width = p.width;
    out->lists = p.lists ? 1 : 0;
    out->reserved = 0;
    out->kept = p.kept;
    out->bytes_down = p.bytes_down;
    out->overrides_up_bytes = p.overrides_up_bytes;
  });
}

void CheckRowBounds(const mi_devop* h, const char* name, const double* row_lb,
                    const double* row_ub, double tolerance) {
  bool ok = row_lb != nullptr && row_ub != nullptr && tolerance >= 0.0 && !std::isinf(tolerance);
  for (int r = 0; ok && r < h->csc.num_rows(); ++r) {
    ok = row_lb[r] == row_lb[r] && row_ub[r] == row_ub[r];
  }
  if (!ok) throw milp::DeviceError(std::string(name) + ": bad bounds or tolerance");
}

int BoundImpliedPanel(mi_devop* h, const double* lbs, const double* ubs, int k,
                      const double* row_lb, const double* row_ub, double* new_lbs,
                      double* new_ubs) {
  return Guard(h, [&] {
    CheckRowBounds(h, "bound_implied_panel", row_lb, row_ub, 0.0);
    h->dev.BoundImpliedPanel(lbs, ubs, k, row_lb, row_ub, new_lbs, new_ubs);
  });
}

int BoundImpliedPanelFrom(mi_devop* h, const double* base_lb, const double* base_ub, int k,
                          const int64_t* starts, const int32_t* cols, const double* ov_lbs,
                          const double* ov_ubs, const double* row_lb, const double* row_ub,
                          double* new_lbs, double* new_ubs) {
  return Guard(h, [&] {
    CheckRowBounds(h, "bound_implied_panel_from", row_lb, row_ub, 0.0);
    CheckBoundOverrides(h, "bound_implied_panel_from", k, starts, cols, ov_lbs, ov_ubs);
    h->dev.BoundImpliedPanelFrom(base_lb, base_ub, k, starts, cols, ov_lbs, ov_ubs, row_lb,
                                 row_ub, new_lbs, new_ubs);
  });
}

// The two filtered entries: run(lists, &result), then the outputs, unless the
// lists need more than `capacity` entries.
template <typename Run>
int TightenedCall(mi_devop* h, const char* name, int k, const double* row_lb,
                  const double* row_ub, double tolerance, int64_t* col_starts, int32_t* cols,
                  double* new_lbs, double* new_ubs, int64_t capacity,
                  mi_devop_point_violations* summaries, Run run) {
  bool too_large = false;
  const int rc = Guard(h, [&] {
    CheckRowBounds(h, name, row_lb, row_ub, tolerance);
    if (col_starts == nullptr && summaries == nullptr) {
      throw milp::DeviceError(std::string(name) + ": no outputs");
    }
    milp::DeviceLp::TightenedColumns result;
    run(col_starts != nullptr, &result);
    if (col_starts != nullptr) {
      const int64_t kept = result.col_starts.back();
      if (kept > capacity) {
        too_large = true;
        throw milp::DeviceError(std::string(name) + ": " + std::to_string(kept) +
                                " entries, capacity " + std::to_string(capacity));
      }
      std::memcpy(col_starts, result.col_starts.data(),
                  result.col_starts.size() * sizeof(int64_t));
      if (kept > 0) {
        std::memcpy(cols, result.cols.data(), size_t(kept) * sizeof(int32_t));
        std::memcpy(new_lbs, result.new_lbs.data(), size_t(kept) * sizeof(double));
        std::memcpy(new_ubs, result.new_ubs.data(), size_t(kept) * sizeof(double));
      }
    }
    if (summaries != nullptr && k > 0) {
      std::memcpy(summaries, result.summaries.data(), size_t(k) * sizeof(*summaries));
    }
  });
  return too_large ? int{MI_DEVOP_CAPACITY} : rc;
}

int BoundTightenedPanel(mi_devop* h, const double* lbs, const double* ubs, int k,
                        const double* row_lb, const double* row_ub, double tolerance,
                        int64_t* col_starts, int32_t* cols, double* new_lbs, double* new_ubs,
                        int64_t capacity, mi_devop_point_violations* summaries) {
  return TightenedCall(h, "bound_tightened_panel", k, row_lb, row_ub, tolerance, col_starts, cols,
                       new_lbs, new_ubs, capacity, summaries,
                       [&](bool lists, milp::DeviceLp::TightenedColumns* out) {
                         h->dev.BoundTightenedPanel(lbs, ubs, k, row_lb, row_ub, tolerance, lists,
                                                    out);
                       });
}

int BoundTightenedPanelFrom(mi_devop* h, const double* base_lb, const double* base_ub, int k,
                            const int64_t* starts, const int32_t* cols_in, const double* ov_lbs,
                            const double* ov_ubs, const double* row_lb, const double* row_ub,
                            double tolerance, int64_t* col_starts, int32_t* cols, double* new_lbs,
                            double* new_ubs, int64_t capacity,
                            mi_devop_point_violations* summaries) {
  return TightenedCall(
      h, "bound_tightened_panel_from", k, row_lb, row_ub, tolerance, col_starts, cols, new_lbs,
      new_ubs, capacity, summaries, [&](bool lists, milp::DeviceLp::TightenedColumns* out) {
        CheckBoundOverrides(h, "bound_tightened_panel_from", k, starts, cols_in, ov_lbs, ov_ubs);
        h->dev.BoundTightenedPanelFrom(base_lb, base_ub, k, starts, cols_in, ov_lbs, ov_ubs,
                                       row_lb, row_ub, tolerance, lists, out);
      });
}

int LastBoundImplied(mi_devop* h, mi_devop_bound_implied* out) {
  return Guard(h, [&] {
    const milp::DeviceLp::LastBoundImplied p = h->dev.last_bound_implied();
    out->panels = p.panels;
    out->width = p.width;
    out->columns = p.columns;
    out->lists = p.lists ? 1 : 0;
    out->kept = p.kept;
    out->bytes_up = p.bytes_up;
    out->bytes_down = p.bytes_down;
  });
}

milp::DeviceLp::PropagateParams CheckPropagateParams(const mi_devop* h, const char* name,
                                                     const mi_devop_propagate_params* p,
                                                     const double* row_lb, const double* row_ub) {
  if (p == nullptr) throw milp::DeviceError(std::string(name) + ": no parameters");
  CheckRowBounds(h, name, row_lb, row_ub, p->tolerance);
  if (p->max_rounds < 1 || !(p->integrality_tolerance >= 0.0) ||
      !(p->integrality_tolerance < 0.5)) {
    throw milp::DeviceError(std::string(name) + ": bad rounds or integrality tolerance");
  }
  return milp::DeviceLp::PropagateParams{p->is_integer, p->tolerance, p->integrality_tolerance,
                                         p->max_rounds};
}

static_assert(sizeof(mi_devop_propagation) == sizeof(mi_lp_propagation) &&
                  sizeof(mi_lp_propagation) == 32 &&
                  offsetof(mi_devop_propagation, moves) == offsetof(mi_lp_propagation, moves) &&
                  offsetof(mi_devop_propagation, worst) == offsetof(mi_lp_propagation, worst) &&
                  offsetof(mi_devop_propagation, worst_col) ==
                      offsetof(mi_lp_propagation, worst_col) &&
                  offsetof(mi_devop_propagation, kept) == offsetof(mi_lp_propagation, kept),
              "mi_lp_devop.h restates mi_lp_propagation");

int BoundPropagatePanel(mi_devop* h, const double* lbs, const double* ubs, int k,
                        const mi_devop_propagate_params* params, const double* row_lb,
                        const double* row_ub, double* new_lbs, double* new_ubs,
                        mi_devop_propagation* summaries) {
  return Guard(h, [&] {
    const milp::DeviceLp::PropagateParams p =
        CheckPropagateParams(h, "bound_propagate_panel", params, row_lb, row_ub);
    if (summaries == nullptr) throw milp::DeviceError("bound_propagate_panel: no summaries");
    h->dev.BoundPropagatePanel(lbs, ubs, k, p, row_lb, row_ub, new_lbs, new_ubs,
                               reinterpret_cast<mi_lp_propagation*>(summaries));
  });
}

int BoundPropagatePanelFrom(mi_devop* h, const double* base_lb, const double* base_ub, int k,
                            const int64_t* starts, const int32_t* cols, const double* ov_lbs,
                            const double* ov_ubs, const mi_devop_propagate_params* params,
                            const double* row_lb, const double* row_ub, double* new_lbs,
                            double* new_ubs, mi_devop_propagation* summaries) {
  return Guard(h, [&] {
    const milp::DeviceLp::PropagateParams p =
        CheckPropagateParams(h, "bound_propagate_panel_from", params, row_lb, row_ub);
    if (summaries == nullptr) throw milp::DeviceError("bound_propagate_panel_from: no summaries");
    CheckBoundOverrides(h, "bound_propagate_panel_from", k, starts, cols, ov_lbs, ov_ubs);
    h->dev.BoundPropagatePanelFrom(base_lb, base_ub, k, starts, cols, ov_lbs, ov_ubs, p, row_lb,
                                   row_ub, new_lbs, new_ubs,
                                   reinterpret_cast<mi_lp_propagation*>(summaries));
  });
}

int BoundPropagatedColumnsFrom(mi_devop* h, const double* base_lb, const double* base_ub, int k,
                               const int64_t* starts, const int32_t* cols_in,
                               const double* ov_lbs, const double* ov_ubs,
                               const mi_devop_propagate_params* params, const double* row_lb,
                               const double* row_ub, int64_t* col_starts, int32_t* cols,
                               double* new_lbs, double* new_ubs, int64_t capacity,
                               mi_devop_propagation* summaries) {
  const char* name = "bound_propagated_columns_from";
  bool too_large = false;
  const int rc = Guard(h, [&] {
    const milp::DeviceLp::PropagateParams p =
        CheckPropagateParams(h, name, params, row_lb, row_ub);
    if (col_starts == nullptr && summaries == nullptr) {
      throw milp::DeviceError(std::string(name) + ": no outputs");
    }
    CheckBoundOverrides(h, name, k, starts, cols_in, ov_lbs, ov_ubs);
    milp::DeviceLp::PropagatedColumns result;
    h->dev.BoundPropagatedColumnsFrom(base_lb, base_ub, k, starts, cols_in, ov_lbs, ov_ubs, p,
                                      row_lb, row_ub, col_starts != nullptr, &result);
    if (col_starts != nullptr) {
      const int64_t kept = result.lists.col_starts.back();
      if (kept > capacity) {
        too_large = true;
        throw milp::DeviceError(std::string(name) + ": " + std::to_string(kept) +
                                " entries, capacity " + std::to_string(capacity));
      }
      std::memcpy(col_starts, result.lists.col_starts.data(),
                  result.lists.col_starts.size() * sizeof(int64_t));
      if (kept > 0) {
        std::memcpy(cols, result.lists.cols.data(), size_t(kept) * sizeof(int32_t));
        std::memcpy(new_lbs, result.lists.new_lbs.data(), size_t(kept) * sizeof(double));
        std::memcpy(new_ubs, result.lists.new_ubs.data(), size_t(kept) * sizeof(double));
      }
    }
    if (summaries != nullptr && k > 0) {
      std::memcpy(summaries, result.summaries.data(), size_t(k) * sizeof(*summaries));
    }
  });
  return too_large ? int{MI_DEVOP_CAPACITY} : rc;
}

int LastBoundPropagate(mi_devop* h, mi_devop_bound_propagate* out) {
  return Guard(h, [&] {
    const milp::DeviceLp::LastBoundPropagate p = h->dev.last_bound_propagate();
    out->panels = p.panels;
    out->width = p.width;
    out->columns = p.columns;
    out->lists = p.lists ? 1 : 0;
    out->rounds = p.rounds;
    out->kept = p.kept;
    out->bytes_up = p.bytes_up;
    out->bytes_down = p.bytes_down;
  });
}

int ColumnPenaltiesPanel(mi_devop* h, const double* y, int k, const double* d,
                         const int8_t* status, const double* unit, const double* down_dist,
                         const double* up_dist, double pivot_tolerance,
                         mi_devop_branch_penalty* out) {
  return Guard(h, [&] {
    if (!milp::DeviceLp::ValidPenaltyArgs(h->csc.num_cols(), k, status, unit, down_dist, up_dist,
                                          pivot_tolerance)) {
      throw milp::DeviceError("column_penalties_panel: bad arguments");
    }
    h->dev.ColumnPenaltiesPanel(y, k, d, reinterpret_cast<const uint8_t*>(status), unit,
                                down_dist, up_dist, pivot_tolerance,
                                reinterpret_cast<mi_lp_branch_penalty*>(out));
  });
}

int LastPenalties(mi_devop* h, mi_devop_penalties* out) {
  return Guard(h, [&] {
    const milp::DeviceLp::LastPenalties p = h->dev.last_penalties();
    out->sparse = p.panel.sparse;
    out->dense = p.panel.dense ? 1 : 0;
    out->panels = p.panel.panels;
    out->width = p.panel.width;
    out->tiles = p.tiles;
    out->reserved = 0;
    out->bytes_down = p.bytes_down;
  });
}

int ColumnCutsPanel(mi_devop* h, const double* y, int k, const int8_t* status,
                    const double* unit, const double* f0, const double* row_unit,
                    double zero_tolerance, double drop_tolerance, int64_t* row_starts,
                    int32_t* cols, double* vals, int64_t capacity,
                    mi_devop_cut_summary* summaries) {
  bool too_large = false;
  const int rc = Guard(h, [&] {
    if (!milp::DeviceLp::ValidCutArgs(h->csc.num_cols(), k, status, unit, f0, row_unit,
                                      zero_tolerance, drop_tolerance)) {
      throw milp::DeviceError("column_cuts_panel: bad arguments");
    }
    milp::DeviceLp::CutRows cuts;
    h->dev.ColumnCutsPanel(y, k, reinterpret_cast<const uint8_t*>(status), unit, f0, row_unit,
                           zero_tolerance, drop_tolerance, row_starts != nullptr, &cuts);
    if (row_starts != nullptr) {
      const int64_t kept = cuts.row_starts.back();
      if (kept > capacity) {
        too_large = true;
        throw milp::DeviceError("column_cuts_panel: " + std::to_string(kept) +
                                " entries, capacity " + std::to_string(capacity));
      }
      std::memcpy(row_starts, cuts.row_starts.data(), cuts.row_starts.size() * sizeof(int64_t));
      if (kept > 0) {
        std::memcpy(cols, cuts.cols.data(), size_t(kept) * sizeof(int32_t));
        std::memcpy(vals, cuts.vals.data(), size_t(kept) * sizeof(double));
      }
    }
    if (summaries != nullptr && k > 0) {
      std::memcpy(summaries, cuts.summaries.data(), size_t(k) * sizeof(mi_lp_cut_summary));
    }
  });
  return too_large ? int{MI_DEVOP_CAPACITY} : rc;
}

int LastCuts(mi_devop* h, mi_devop_cuts* out) {
  return Guard(h, [&] {
    const milp::DeviceLp::LastCuts p = h->dev.last_cuts();
    out->sparse = p.panel.sparse;
    out->dense = p.panel.dense ? 1 : 0;
    out->panels = p.panel.panels;
    out->width = p.panel.width;
    out->tiles = p.tiles;
    out->structural_tiles = p.structural_tiles;
    out->lists = p.lists ? 1 : 0;
    out->reserved = 0;
    out->kept = p.kept;
    out->bytes_down = p.bytes_down;
  });
}

// --- triangular solves ------------------------------------------------------

int TriCols(const mi_devop* h) {
  if (h->tri.IsEmpty()) throw milp::DeviceError("no triangular matrix: tri_set_matrix first");
  return h->tri.num_cols();
}

milp::TriKind TriKindOf(int kind) {
  if (kind < 0 || kind >= milp::kNumTriKinds) throw milp::DeviceError("bad triangular kind");
  return static_cast<milp::TriKind>(kind);
}

int TriSetMatrix(mi_devop* h, int n, const int64_t* col_starts, const int32_t* rows,
                 const double* vals, const double* diag) {
  return Guard(h, [&] {
    if (n < 1 || col_starts == nullptr || diag == nullptr || col_starts[0] != 0) {
      throw milp::DeviceError("tri_set_matrix: bad arguments");
    }
    for (int c = 0; c < n; ++c) {
      if (col_starts[c + 1] < col_starts[c]) {
        throw milp::DeviceError("tri_set_matrix: column starts descend");
      }
      for (int64_t i = col_starts[c]; i < col_starts[c + 1]; ++i) {
        if (rows[i] < 0 || rows[i] >= n || rows[i] == c) {
          throw milp::DeviceError("tri_set_matrix: row out of range or on the diagonal");
        }
      }
    }
    // The async solve and the dense tail read the matrix being replaced.
    h->dev.DropAsyncU();
    h->tri.Reset(n, n);
    std::vector<int> r;
    std::vector<double> v;
    for (int c = 0; c < n; ++c) {
      r.assign(rows + col_starts[c], rows + col_starts[c + 1]);
      v.assign(vals + col_starts[c], vals + col_starts[c + 1]);
      r.push_back(c);
      v.push_back(diag[c]);
      milp::ColumnView view;
      view.rows = r.data();
      view.coefs = v.data();
      view.n = static_cast<int64_t>(r.size());
      h->tri.AddTriangularColumn(view, c);
    }
  });
}

int TriSolve(mi_devop* h, int kind, uint64_t key, int start, double* x, int* on_device) {
  return Guard(h, [&] {
    const int n = TriCols(h);
    std::vector<double> v(x, x + n);
    *on_device = h->dev.Solve(TriKindOf(kind), h->tri, key, start, &v) ? 1 : 0;
    if (*on_device != 0) std::memcpy(x, v.data(), size_t(n) * sizeof(double));
  });
}

int TriSolvePair(mi_devop* h, int kind, uint64_t key, double* x0, double* x1, int* on_device) {
  return Guard(h, [&] {
    const int n = TriCols(h);
    std::vector<double> v0(x0, x0 + n), v1(x1, x1 + n);
    *on_device = h->dev.SolvePair(TriKindOf(kind), h->tri, key, &v0, &v1) ? 1 : 0;
    if (*on_device != 0) {
      std::memcpy(x0, v0.data(), size_t(n) * sizeof(double));
      std::memcpy(x1, v1.data(), size_t(n) * sizeof(double));
    }
  });
}

int TriAsyncBegin(mi_devop* h, uint64_t key, const double* x, int* started) {
  return Guard(h, [&] {
    const std::vector<double> v(x, x + TriCols(h));
    *started = h->dev.StartAsyncU(h->tri, key, v) ? 1 : 0;
  });
}

int TriAsyncFinish(mi_devop* h, double* x) {
  return Guard(h, [&] {
    const int n = TriCols(h);
    std::vector<double> v(x, x + n);
    h->dev.FinishAsyncU(&v);
    std::memcpy(x, v.data(), size_t(n) * sizeof(double));
  });
}

int TriAsyncDrop(mi_devop* h) {
  return Guard(h, [&] { h->dev.DropAsyncU(); });
}

int TriHostSolve(mi_devop* h, int kind, int start, double* x) {
  return Guard(h, [&] {
    const int n = TriCols(h);
    std::vector<double> v(x, x + n);
    switch (TriKindOf(kind)) {
      case milp::TriKind::kUpperT:
      case milp::TriKind::kLowerT:
        h->tri.TransposeLowerSolve(&v);
        break;
      case milp::TriKind::kUpperTUp:
        h->tri.TransposeUpperSolve(&v);
        break;
      case milp::TriKind::kLower:
      case milp::TriKind::kUnitRow:
        if (start < 0 || start > n) throw milp::DeviceError("tri_host_solve: bad start");
        h->tri.LowerSolveStartingAt(start, &v);
        break;
      case milp::TriKind::kUpper:
        h->tri.UpperSolve(&v);
        break;
    }
    std::memcpy(x, v.data(), size_t(n) * sizeof(double));
  });
}

int LastTri(mi_devop* h, mi_devop_tri* out) {
  return Guard(h, [&] {
    const milp::DeviceLp::LastTri p = h->dev.last_tri();
    out->plan = p.plan;
    out->kind = p.kind;
    out->rows = p.rows;
    out->first_col = p.first_col;
    out->top = p.top;
    out->work = p.work;
    out->pos = p.pos;
    out->levels = p.levels;
    out->chain_levels = p.chain_levels;
    out->level0_end = p.level0_end;
    out->wide_runs = p.wide_runs;
    out->chain_runs = p.chain_runs;
    out->chip_launches = p.chip_launches;
    out->cu_runs = p.cu_runs;
    out->fused0 = p.fused0 ? 1 : 0;
    out->vectors = p.vectors;
    out->max_wide_run = p.max_wide_run;
    out->max_entries = p.max_entries;
    for (int i = 0; i < 3; ++i) out->rows_over[i] = p.rows_over[i];
    out->t = p.t;
    out->tail_cols = p.tail_cols;
    out->blocks = p.blocks;
    out->entries = p.entries;
  });
}

int LastTriLevelWidths(mi_devop* h, int32_t* widths, int capacity, int* count) {
  return Guard(h, [&] {
    const std::vector<int32_t> w = h->dev.last_tri_level_widths();
    *count = static_cast<int>(w.size());
    const size_t k = std::min<size_t>(w.size(), capacity > 0 ? size_t(capacity) : 0);
    if (k > 0) std::memcpy(widths, w.data(), k * sizeof(int32_t));
  });
}

int AppendRows(mi_devop* h, int k, const int64_t* row_starts, const int32_t* cols,
               const double* vals) {
  return Guard(h, [&] {
    const int n = h->csc.num_cols() - h->csc.num_rows();
    if (k < 0 || row_starts == nullptr || !milp::ValidRowLists(n, k, row_starts, cols, vals)) {
      throw milp::DeviceError("append_rows: bad row lists");
    }
    h->csc.AppendRows(n, k, row_starts, cols, vals);
    h->csr.AppendTransposedRows(k, row_starts, cols, vals);
    h->dev.AppendRows(h->csc, h->csr, k);
    h->relevant.assign((h->csc.num_cols() + 63) / 64, ~0ull);
  });
}

int FetchMatrix(mi_devop* h, int64_t* starts, int32_t* rows, double* vals, int64_t* t_starts,
                int32_t* t_cols, double* t_vals, int32_t* nd, int32_t* dense_cols,
                double* dense_block, int64_t capacity) {
  int rc = 0;
  const int guarded = Guard(h, [&] {
    milp::DeviceLp::MatrixCopy c;
    h->dev.FetchMatrix(&c);
    if (static_cast<int64_t>(c.starts.size()) != h->csc.num_cols() + 1 ||
        static_cast<int64_t>(c.rows.size()) != h->csc.num_entries()) {
      throw milp::DeviceError("fetch_matrix: the device's shape is not the handle's");
    }
    *nd = static_cast<int32_t>(c.dense_cols.size());
    if (static_cast<int64_t>(c.dense_block.size()) > capacity) {
      rc = MI_DEVOP_CAPACITY;
      return;
    }
    const auto put = [](void* dst, const void* src, size_t bytes) {
      if (bytes > 0) std::memcpy(dst, src, bytes);
    };
    put(starts, c.starts.data(), c.starts.size() * sizeof(int64_t));
    put(rows, c.rows.data(), c.rows.size() * sizeof(int32_t));
    put(vals, c.vals.data(), c.vals.size() * sizeof(double));
    put(t_starts, c.t_starts.data(), c.t_starts.size() * sizeof(int64_t));
    put(t_cols, c.t_cols.data(), c.t_cols.size() * sizeof(int32_t));
    put(t_vals, c.t_vals.data(), c.t_vals.size() * sizeof(double));
    put(dense_cols, c.dense_cols.data(), c.dense_cols.size() * sizeof(int32_t));
    put(dense_block, c.dense_block.data(), c.dense_block.size() * sizeof(double));
  });
  return guarded != 0 ? guarded : rc;
}

int LastAppend(mi_devop* h, mi_devop_append* out) {
  return Guard(h, [&] {
    const milp::DeviceLp::LastAppend p = h->dev.last_append();
    out->path = p.path;
    out->rows = p.rows;
    out->entries = p.entries;
    out->bytes_up = p.bytes_up;
    out->move_shapes = p.move_shapes;
    out->reserved = 0;
    out->device_ms = p.device_ms;
  });
}

int DeleteRows(mi_devop* h, const uint8_t* delete_mask) {
  return Guard(h, [&] {
    const int m = h->csc.num_rows();
    const int n = h->csc.num_cols() - m;
    if (delete_mask == nullptr && m > 0) throw milp::DeviceError("delete_rows: no mask");
    const std::vector<int> new_row = milp::NewRowIndices(m, delete_mask);
    h->csc.DeleteRows(n, delete_mask, new_row.data());
    h->csr.DeleteTransposedRows(n, delete_mask, new_row.data());
    h->dev.DeleteRows(h->csc, h->csr, delete_mask);
    h->relevant.assign((h->csc.num_cols() + 63) / 64, ~0ull);
  });
}

int LastDelete(mi_devop* h, mi_devop_delete* out) {
  return Guard(h, [&] {
    const milp::DeviceLp::LastDelete p = h->dev.last_delete();
    out->path = p.path;
    out->rows = p.rows;
    out->entries = p.entries;
    out->bytes_up = p.bytes_up;
    out->column_shapes = p.column_shapes;
    out->row_shapes = p.row_shapes;
    out->device_ms = p.device_ms;
  });
}

static_assert(int{MI_DEVOP_TRI_UPPER} == static_cast<int>(milp::TriKind::kUpper) &&
                  int{MI_DEVOP_TRI_UNIT_ROW} == static_cast<int>(milp::TriKind::kUnitRow) &&
                  int{MI_DEVOP_TRI_UPPER_T_UP} == static_cast<int>(milp::TriKind::kUpperTUp),
              "mi_lp_devop.h restates TriKind");
static_assert(int{MI_DEVOP_TRI_PLAN_DENSE_TAIL} == int{milp::DeviceLp::kTriPlanDenseTail} &&
                  int{MI_DEVOP_TRI_PLAN_LEVELS} == int{milp::DeviceLp::kTriPlanLevels},
              "mi_lp_devop.h restates DeviceLp's triangular plans");
static_assert(sizeof(mi_devop_cut_summary) == sizeof(mi_lp_cut_summary) &&
                  offsetof(mi_devop_cut_summary, min_col) == offsetof(mi_lp_cut_summary, min_col),
              "mi_lp_devop.h restates mi_lp_cut_summary");
static_assert(sizeof(mi_devop_branch_penalty) == sizeof(mi_lp_branch_penalty) &&
                  offsetof(mi_devop_branch_penalty, up_count) ==
                      offsetof(mi_lp_branch_penalty, up_count),
              "mi_lp_devop.h restates mi_lp_branch_penalty");
static_assert(sizeof(mi_devop_point_violations) == sizeof(mi_lp_point_violations) &&
                  offsetof(mi_devop_point_violations, worst_row) ==
                      offsetof(mi_lp_point_violations, worst_row),
              "mi_lp_devop.h restates mi_lp_point_violations");
static_assert(int{MI_DEVOP_ROW_PANEL_DIRECT} == int{milp::DeviceLp::kRowPanelDirect},
              "mi_lp_devop.h restates DeviceLp's row panel paths");
static_assert(int{MI_DEVOP_PANEL_LONG_COLUMNS} == int{milp::DeviceLp::kPanelLongColumns},
              "mi_lp_devop.h restates DeviceLp's panel shapes");
static_assert(int{MI_DEVOP_ROW_COLUMN_WISE_GENERAL} == int{milp::DeviceLp::kRowColumnWiseGeneral} &&
                  int{MI_DEVOP_ROW_LIST} == int{milp::DeviceLp::kRowList} &&
                  int{MI_DEVOP_COMPACT_CHIP_WIDE} == int{milp::DeviceLp::kCompactChipWide} &&
                  int{MI_DEVOP_RATIO_TWO_KERNELS} == int{milp::DeviceLp::kRatioTwoKernels},
              "mi_lp_devop.h restates DeviceLp's path enums");

}  // namespace

extern "C" const mi_devop_api mi_devop_table = {
    Create,           Destroy,
    LastError,        SetMask,
    SetListMirror,    SetSmallBatch,
    UpdateRowRowWise, UpdateRowColumnWise,
    FetchUpdateRow,   ReadCoefficient,
    DownloadCoefficients, ListDotsOverUpdateRow,
    ListDots,         DualBegin,
    DualSetColBits,   DualRatioCandidates,
    DualUpdateReducedCosts, DualDownloadReducedCosts,
    LastPaths,
    ColumnDotsPanel,  LastPanel,
    TakeKernelMs,
    ColumnDotsPanelSparse, LastPanelSparse,
    PanelSparseGeometry,
    Pricing,          ColumnSquaredNorms,
    RowSums,          DualBoxedFlips,
    DualBoxedFlipsEarly, DualTakePricedReducedCosts,
    DualSetReducedCost, LastColumnDots,
    LastFlips,
    RowSumsPanel,     RowSumsPanelFrom,
    LastRowPanel,     RowPanelGeometry,
    RowViolationsPanel, RowViolationsPanelFrom,
    LastRowViolations,
    BoundRangesPanel, BoundRangesPanelFrom,
    BoundInfeasiblePanel, BoundInfeasiblePanelFrom,
    LastBoundRanges,
    BoundImpliedPanel, BoundImpliedPanelFrom,
    BoundTightenedPanel, BoundTightenedPanelFrom,
    LastBoundImplied,
    BoundPropagatePanel, BoundPropagatePanelFrom,
    BoundPropagatedColumnsFrom,
    LastBoundPropagate,
    ColumnPenaltiesPanel, LastPenalties,
    ColumnCutsPanel, LastCuts,
    TriSetMatrix,     TriSolve,
    TriSolvePair,     TriAsyncBegin,
    TriAsyncFinish,   TriAsyncDrop,
    TriHostSolve,     LastTri,
    LastTriLevelWidths,
};

extern "C" const mi_devop_matrix_api mi_devop_matrix_table = {
    AppendRows,
    FetchMatrix,
    LastAppend,
};

extern "C" const mi_devop_matrix_delete_api mi_devop_matrix_delete_table = {
    DeleteRows,
    LastDelete,
};
