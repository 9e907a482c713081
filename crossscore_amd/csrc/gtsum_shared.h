// The closing reduction of the two frame-sum kernels (gtsum.hip, and the sums form of gt_ssim_kernel in gtmap.hip): every thread's share of
// the four integer sums S1..S4 of its frame (include/crossscore_hip.h, cs_op_metric_map_sums_u16) -> four 64-bit atomic adds per workgroup.
// Unsigned integer addition: the result does not depend on the order of the shuffles, the waves or the atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// v[k]: this thread's share of S(k+1), 0 for a thread that owns no pixel.  red: kWaves x 4 words of LDS.  slot: the frame's four sums.
// Holds a workgroup barrier: every thread of the workgroup calls it, none may have left before.
template <int kWaves>
__device__ __forceinline__ void cs_sums_block_add(const unsigned long long (&v)[4], unsigned long long (*red)[4], unsigned long long* slot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    unsigned long long s = v[k];
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      unsigned long long s = 0;
      for (int w = 0; w < kWaves; ++w) s += red[w][k];
      atomicAdd(slot + k, s);
    }
  }
}
