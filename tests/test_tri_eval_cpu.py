"""The evaluation rules of the dense triangular solve (kernels/tri_eval.h,
used by every kernel of kernels/tri_solve.hip) against Glop's loops written
out directly: TransposeLowerSolve's grouped sums (sparse.cc:899-955) and
LowerSolveStartingAt's one subtraction per entry with its zero skip
(sparse.cc:793-812). The header is plain C++ under g++: a stand-alone
program, no GPU, no engine library. Bit equality throughout."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = r"""
#include "tri_eval.h"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>
using milp_kernels::kTriPending;
using milp_kernels::tri_finish;
using milp_kernels::tri_fold_window;
using milp_kernels::tri_pending;
using milp_kernels::tri_pending_mark;
using milp_kernels::tri_short;

static uint64_t g_state = SEED;
static uint64_t Next() {  // splitmix64
  uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
// Magnitudes spread over 2^-20 .. 2^20, mixed signs.
static double Value() {
  const double m = 1.0 + static_cast<double>(Next() >> 11) / 9007199254740992.0;
  const int e = static_cast<int>(Next() % 41) - 20;
  return std::ldexp((Next() & 1) ? m : -m, e);
}
static uint64_t Bits(double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  return b;
}
static double FromBits(uint64_t b) {
  double v;
  std::memcpy(&v, &b, 8);
  return v;
}

// Glop's loops, seen from one output.
static double RefGrouped(double sum, int n, const double* w, const double* y) {
  int i = 0;
  for (; i + 3 < n; i += 4) {
    sum -= w[i] * y[i] + w[i + 1] * y[i + 1] + w[i + 2] * y[i + 2] + w[i + 3] * y[i + 3];
  }
  for (; i < n; ++i) sum -= w[i] * y[i];
  return sum;
}
static double RefSequential(double sum, int n, const double* w, const double* y) {
  for (int i = 0; i < n; ++i) {
    if (y[i] == 0.0) continue;  // the host skips that column
    sum -= y[i] * w[i];
  }
  return sum;
}
static double OneByOne(double sum, int n, const double* w, const double* y) {
  for (int i = 0; i < n; ++i) sum -= w[i] * y[i];
  return sum;
}
static double RefFinish(bool sequential, bool has_diag, double sum, double d) {
  if (!has_diag) return sum;
  if (sequential && sum == 0.0) return sum;  // a zero column is skipped, not divided
  return sum / d;
}

static int g_fail = 0;
static void Fail(const char* what, int n, int seq, int extra) {
  if (++g_fail <= 20) std::printf("FAIL %s n=%d sequential=%d (%d)\n", what, n, seq, extra);
}

// Entry i's input is final from step arrival[i] on. As the kernels do: windows
// of the next up-to-8 entries, again at once after a whole window, else the
// next step.
static double Drive(bool seq, double sum, int n, const double* w, const double* y,
                    const std::vector<int>& arrival, bool* ok) {
  int e = 0;
  for (int step = 0; e < n; ++step) {
    if (step > n + 1) {  // every input is final by step n - 1
      *ok = false;
      return sum;
    }
    while (e < n) {
      double ww[8], vv[8];
      for (int i = 0; i < 8; ++i) {
        const bool in = e + i < n;
        ww[i] = in ? w[e + i] : 0.0;
        vv[i] = !in ? 0.0 : arrival[e + i] <= step ? y[e + i] : tri_pending_mark();
      }
      const uint64_t before = Bits(sum);
      const int took = tri_fold_window(seq, n - e, ww, vv, &sum);
      if (took < 0 || took > 8 || e + took > n) *ok = false;
      if (took == 0 && Bits(sum) != before) *ok = false;  // nothing taken: untouched
      for (int i = 0; i < took; ++i) {
        if (arrival[e + i] > step) *ok = false;  // took an input that was not final
      }
      if (!*ok) return sum;
      e += took;
      if (took < 8) break;
    }
  }
  return sum;
}

static void TestFold() {
  const int kSets = 8;
  for (int n = 5; n <= 41; ++n) {
    int regrouped_differs[2] = {0, 0};
    for (int set = 0; set < kSets; ++set) {
      std::vector<double> w(n), y(n);
      for (int i = 0; i < n; ++i) {
        w[i] = Value();
        y[i] = Value();
      }
      const double sum0 = Value();
      for (int seq = 0; seq < 2; ++seq) {
        // The sequential form's zero skip: a few zero inputs, of both signs.
        std::vector<double> yy = y;
        if (seq) {
          yy[Next() % n] = 0.0;
          yy[Next() % n] = -0.0;
        }
        const double ref = seq ? RefSequential(sum0, n, w.data(), yy.data())
                               : RefGrouped(sum0, n, w.data(), yy.data());
        // The other grouping of the same terms must be able to differ.
        const double other = seq ? RefGrouped(sum0, n, w.data(), yy.data())
                                 : OneByOne(sum0, n, w.data(), yy.data());
        if (n >= 6 && Bits(other) != Bits(ref)) ++regrouped_differs[seq];
        std::vector<int> arrival(n, 0);
        for (int sched = 0; sched < 53; ++sched) {
          if (sched == 1) {
            std::iota(arrival.begin(), arrival.end(), 0);
          } else if (sched == 2) {
            for (int i = 0; i < n; ++i) arrival[i] = n - 1 - i;
          } else if (sched >= 3) {  // a seeded random arrival order
            std::iota(arrival.begin(), arrival.end(), 0);
            for (int i = n - 1; i > 0; --i) std::swap(arrival[i], arrival[Next() % (i + 1)]);
          }
          bool ok = true;
          const double got = Drive(seq != 0, sum0, n, w.data(), yy.data(), arrival, &ok);
          if (!ok) Fail("fold step", n, seq, sched);
          if (Bits(got) != Bits(ref)) Fail("fold bits", n, seq, sched);
        }
      }
    }
    if (n >= 6) {
      for (int seq = 0; seq < 2; ++seq) {
        if (regrouped_differs[seq] == 0) Fail("condition: regrouping never changes the bits", n, seq, 0);
      }
    }
  }
}

static double Short(bool seq, bool has_diag, int n, double sum, const double* w, const double* y,
                    double d) {
  double v[4], yy[4];
  for (int i = 0; i < 4; ++i) {
    v[i] = i < n ? w[i] : 0.0;
    yy[i] = i < n ? y[i] : 0.0;
  }
  return tri_finish(seq, has_diag, tri_short(seq, n, sum, v, yy[0], yy[1], yy[2], yy[3]), d);
}

static void TestShort() {
  for (int rep = 0; rep < 200; ++rep) {
    for (int n = 0; n <= 4; ++n) {
      for (int seq = 0; seq < 2; ++seq) {
        for (int has_diag = 0; has_diag < 2; ++has_diag) {
          double w[4], y[4];
          for (int i = 0; i < 4; ++i) {
            w[i] = Value();
            y[i] = Value();
          }
          if (n > 0 && rep % 3 == 1) y[Next() % n] = 0.0;
          if (n > 0 && rep % 3 == 2) y[Next() % n] = -0.0;
          double sum0 = Value();
          if (rep % 5 == 3) sum0 = 0.0;
          if (rep % 5 == 4) sum0 = -0.0;
          const double d = Value();
          const double body = seq ? RefSequential(sum0, n, w, y) : RefGrouped(sum0, n, w, y);
          const double ref = RefFinish(seq != 0, has_diag != 0, body, d);
          const double got = Short(seq != 0, has_diag != 0, n, sum0, w, y, d);
          if (Bits(got) != Bits(ref)) Fail("short bits", n, seq, has_diag);
        }
      }
    }
  }
  // A zero sum of the sequential form is not divided and keeps its sign bit;
  // the grouped form divides it.
  const double w[4] = {0, 0, 0, 0}, y[4] = {0, 0, 0, 0};
  if (Bits(Short(true, true, 0, -0.0, w, y, -2.0)) != Bits(-0.0)) Fail("-0 sequential", 0, 1, 0);
  if (Bits(Short(true, true, 0, 0.0, w, y, -2.0)) != Bits(0.0)) Fail("+0 sequential", 0, 1, 0);
  if (Bits(Short(false, true, 0, -0.0, w, y, -2.0)) != Bits(0.0)) Fail("-0 grouped", 0, 0, 0);
  if (Bits(Short(true, false, 0, 3.0, w, y, 2.0)) != Bits(3.0)) Fail("no diagonal", 0, 1, 0);
  if (Bits(Short(false, false, 0, 3.0, w, y, 2.0)) != Bits(3.0)) Fail("no diagonal", 0, 0, 0);
  // The sum reaches zero through its entries: 1 - 1 * 1.
  const double w1[4] = {1, 0, 0, 0}, y1[4] = {1, 0, 0, 0};
  if (Bits(Short(true, true, 1, 1.0, w1, y1, -2.0)) != Bits(0.0)) Fail("0 by entries", 1, 1, 0);
  if (Bits(Short(false, true, 1, 1.0, w1, y1, -2.0)) != Bits(-0.0)) Fail("0 by entries", 1, 0, 0);
}

static void TestPending() {
  if (!tri_pending(FromBits(kTriPending))) Fail("the mark is pending", 0, 0, 0);
  if (!tri_pending(tri_pending_mark())) Fail("the mark is pending", 0, 0, 1);
  const uint64_t finals[] = {0x7ff8000000000000ull, 0xfff8000000000000ull, kTriPending + 1,
                             kTriPending | 0x8000000000000000ull, 0x7ff0000000000000ull, 0};
  for (uint64_t b : finals) {
    if (tri_pending(FromBits(b))) Fail("a final value counts as pending", 0, 0, 2);
  }
  for (int seq = 0; seq < 2; ++seq) {
    // A quiet NaN input is final: the whole output of 5 folds (to NaN).
    double w[8] = {1, 2, 3, 4, 5, 0, 0, 0};
    double v[8] = {1, 1, FromBits(0x7ff8000000000000ull), 1, 1, 0, 0, 0};
    double sum = 1.0;
    if (tri_fold_window(seq != 0, 5, w, v, &sum) != 5 || sum == sum) Fail("NaN input", 5, seq, 0);
    // The mark at entry 5 of 9: the grouped form stops after the first group,
    // the sequential one after entry 4.
    double w9[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    double v9[8] = {1, 1, 1, 1, 1, tri_pending_mark(), 1, 1};
    sum = 100.0;
    const int took = tri_fold_window(seq != 0, 9, w9, v9, &sum);
    if (took != (seq ? 5 : 4) || sum != (seq ? 85.0 : 90.0)) Fail("mark in window", 9, seq, took);
    // The mark first: nothing taken, the sum untouched.
    v9[0] = tri_pending_mark();
    sum = 100.0;
    if (tri_fold_window(seq != 0, 9, w9, v9, &sum) != 0 || Bits(sum) != Bits(100.0)) {
      Fail("mark first", 9, seq, 0);
    }
  }
}

int main() {
  TestFold();
  TestShort();
  TestPending();
  if (g_fail != 0) {
    std::printf("%d failures\n", g_fail);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
"""

# A condition on the inputs: for every n in 6..41 and both forms, regrouping
# the terms (one by one instead of by fours, and the reverse) changes the bits
# of at least one of the 8 value sets, so the equalities checked can fail. The
# program fails if the seed does not satisfy it; this one does.
SEED = 1


def test_tri_eval_matches_glop_loops(tmp_path):
    src = tmp_path / "tri_eval_test.cc"
    src.write_text(PROG)
    exe = tmp_path / "tri_eval_test"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", f"-DSEED={SEED}ull",
                    "-I", os.path.join(REPO, "or-tools_amd", "csrc", "kernels"), str(src),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok", r.stdout
