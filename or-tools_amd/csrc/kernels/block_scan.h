// The block-wide scan shared by every kernel that places list entries in
// order (simplex_kernels.hip's update-row lists, panel_kernels.hip's sparse
// rows): one definition ("What the update-row kernels share").
#pragma once
#include <hip/hip_runtime.h>

#include "kernel_args.h"

namespace milp_kernels {

constexpr int kWave = 64;

// Block-wide exclusive scan of one int per thread (THREADS threads, all of
// them call it); *total = the sum over the block. lds_waves holds THREADS /
// kWave ints. The only barrier sits between writing and reading lds_waves:
// a caller that scans twice through the same lds_waves owns a barrier between
// the two calls (a slow wave may still be reading the first call's sums).
template <int THREADS = kScanThreads>
__device__ __forceinline__ int scan_block_exclusive(int c, int* total, int* lds_waves) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  int x = c;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int y = __shfl_up(x, off, kWave);
    if (lane >= off) x += y;
  }
  if (lane == kWave - 1) lds_waves[wave] = x;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < THREADS / kWave; ++w) {
    const int v = lds_waves[w];
    before += w < wave ? v : 0;
    all += v;
  }
  *total = all;
  return before + x - c;
}

}  // namespace milp_kernels
