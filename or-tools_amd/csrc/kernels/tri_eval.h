// Evaluation rules of one output of a dense triangular solve (tri_solve.hip):
// the only place where the operation order that gives Glop's bits is written.
//
// Two forms. Grouped (TransposeLowerSolve / TransposeUpperSolve, sparse.cc:
// 848-955): the products of four entries summed left to right and subtracted
// as one group, group after group in list order, then the 1-3 remaining
// products one by one; the result divided by the diagonal if there is one.
// Sequential (LowerSolveStartingAt / UpperSolve seen from one output,
// sparse.cc:792-846): one subtraction per entry in list order, an entry whose
// input is zero contributes nothing (the host skips that column); a zero
// result keeps its bits and is not divided.
//
// Arithmetic on the values handed in only: no memory access beyond the
// argument arrays, no HIP builtins, so the host compiler builds it too
// (tests/test_tri_eval_cpu.py).
#pragma once

#ifdef __HIPCC__
#define TRI_EVAL_FN __host__ __device__ __forceinline__
#else
#define TRI_EVAL_FN inline
#endif

namespace milp_kernels {

// The value of an output that is not final yet: a NaN no arithmetic makes.
// Every other value, the other NaNs included, is final.
constexpr unsigned long long kTriPending = 0x7ff0deadbeef0001ull;

TRI_EVAL_FN bool tri_pending(double v) {
  unsigned long long bits;
  __builtin_memcpy(&bits, &v, sizeof(bits));
  return bits == kTriPending;
}

TRI_EVAL_FN double tri_pending_mark() {
  const unsigned long long bits = kTriPending;
  double v;
  __builtin_memcpy(&v, &bits, sizeof(v));
  return v;
}

// The output from its sum after every entry was subtracted.
TRI_EVAL_FN double tri_finish(bool sequential, bool has_diag, double sum, double d) {
  if (sequential) return (has_diag && sum != 0.0) ? sum / d : sum;
  return has_diag ? sum / d : sum;
}

// The grouped form's step: four products summed left to right, subtracted as
// one group.
TRI_EVAL_FN double tri_sub_group(double sum, double w0, double y0, double w1, double y1,
                                 double w2, double y2, double w3, double y3) {
  return sum - (w0 * y0 + w1 * y1 + w2 * y2 + w3 * y3);
}

// The sequential form's step: an entry whose input is zero contributes nothing.
TRI_EVAL_FN double tri_sub_skip(double sum, double w, double y) {
  return y != 0.0 ? sum - y * w : sum;
}

// An output of n <= 4 entries: `sum` less its entries (values v, inputs
// y0..y3, all final; 0.0 for the entries past n).
TRI_EVAL_FN double tri_short(bool sequential, int n, double sum, const double v[4], double y0,
                             double y1, double y2, double y3) {
  if (sequential) {
    sum = tri_sub_skip(sum, v[0], y0);
    sum = tri_sub_skip(sum, v[1], y1);
    sum = tri_sub_skip(sum, v[2], y2);
    return tri_sub_skip(sum, v[3], y3);
  }
  if (n == 4) {
    sum = tri_sub_group(sum, v[0], y0, v[1], y1, v[2], y2, v[3], y3);
  } else {
    if (n > 0) sum -= v[0] * y0;
    if (n > 1) sum -= v[1] * y1;
    if (n > 2) sum -= v[2] * y2;
  }
  return sum;
}

// One step of the fold of an output of more than 4 entries. `left` entries
// remain; w[i] and v[i] are the value and the input of the next min(left, 8)
// of them, an input that is not final being the pending mark. Subtracts from
// *sum what can be taken now, in evaluation order, and returns how many
// entries that was (0: *sum untouched). Grouped: the window's first group of
// four if its inputs are final, then its second likewise; the last 1-3
// entries of the output, when they are all in the window and final, one by
// one. Sequential: entries up to the first pending one. w[i] is read only for
// an entry that is taken (i < left), so w may point into an entry array.
TRI_EVAL_FN int tri_fold_window(bool sequential, int left, const double w[8], const double v[8],
                                double* sum) {
  int took = 0;
  if (sequential) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (took != i || i >= left || tri_pending(v[i])) continue;
      *sum = tri_sub_skip(*sum, w[i], v[i]);
      took = i + 1;
    }
    return took;
  }
#pragma unroll
  for (int g = 0; g < 8; g += 4) {
    if (took != g || g + 3 >= left) continue;
    if (tri_pending(v[g]) || tri_pending(v[g + 1]) || tri_pending(v[g + 2]) ||
        tri_pending(v[g + 3])) {
      continue;
    }
    *sum = tri_sub_group(*sum, w[g], v[g], w[g + 1], v[g + 1], w[g + 2], v[g + 2], w[g + 3],
                         v[g + 3]);
    took = g + 4;
  }
  const int tail = left - took;
  if (took < 8 && tail > 0 && tail < 4) {
    const int t = took;
    bool ready = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (i < tail && t + i < 8) ready = ready && !tri_pending(v[t + i]);
    }
    if (ready && t + tail <= 8) {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        if (i < tail) *sum -= w[t + i] * v[t + i];
      }
      took = t + tail;
    }
  }
  return took;
}

}  // namespace milp_kernels
