// The fixed-point int64 accumulator under the reproducible scatters, stated once: PWC-Net's and SpyNet's warp backward and
// FlowNet2's Resample2d backward (warp_ops.hip), the on-demand RAFT/GMA correlation's backward (corr_ondemand.hip).
//   - Contributions are added as integers.  Integer adds commute and associate, so the order in which the atomics land
//     cannot change a sum: two runs, two processes, one pair or several in flight give the same bits.
//   - The unit of a call is 2^-shift.  shift comes from the call's max|x| (block maxima, re-reduced: a maximum does not
//     depend on the order either); HOW MANY bits it budgets is each caller's policy and stays with its kernel.
//   - A non-finite value has no fixed-point image (fmaxf drops NaN, the conversion to int64 saturates).  A block that meets
//     Inf, NaN or |x| > 3.0e38 stores +inf as its maximum, and that flags the whole call: shift = FIX_NONFINITE.
//   - A flagged call never scatters a meaningful value (its scale is 0, or its scatter is skipped), and its conversion
//     writes quiet NaN into EVERY output: a superset of what the fp32 operator would poison, never finite garbage.
#pragma once
#include "common.hpp"

constexpr int FIX_NONFINITE = -(1 << 20);   // the shift of a flagged call
__device__ __forceinline__ float fix_inf() { return __int_as_float(0x7f800000); }
__device__ __forceinline__ float fix_qnan() { return __int_as_float(0x7fc00000); }
// the flag rule, for an element and for a maximum alike (NaN fails the comparison too)
__device__ __forceinline__ bool fix_has_image(float absv) { return absv <= 3.0e38f; }

// bmax[blockIdx.x] = max |x| over this block's grid-stride share of x[0, n), +inf for the flag.  each(i) runs before
// element i is read: the pass that clears accumulators of the same count.  red: 4 floats of LDS.
template <class Each>
__device__ __forceinline__ void fix_absmax_share(const float* __restrict__ x, long long n, float* __restrict__ bmax,
                                                 float* red, Each each) {
  const long long step = (long long)gridDim.x * blockDim.x;
  float m = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    each(i);
    const float v = fabsf(x[i]);
    m = fix_has_image(v) ? fmaxf(m, v) : fix_inf();
  }
  m = block_max_256(m, red);
  if (threadIdx.x == 0) bmax[blockIdx.x] = m;
}

// max |x| of the call from its nblk block maxima: a thread's share, then the maximum on every thread of a 256-thread block,
// +inf for a flagged call (two steps: a kernel with two maxima loads both before it reduces either)
__device__ __forceinline__ float fix_bmax_share(const float* __restrict__ bmax, int nblk) {
  float m = 0.f;
  for (int i = threadIdx.x; i < nblk; i += 256) m = fmaxf(m, bmax[i]);
  return m;
}
__device__ __forceinline__ float fix_block_absmax(float share, float* red) {
  const float m = block_max_256(share, red);
  return fix_has_image(m) ? m : fix_inf();
}

// v in units of 1 / scale (scale = 2^shift), rounded to nearest once; two's complement, so that unsigned adds sum it
__device__ __forceinline__ unsigned long long fix_quantize(float v, double scale) {
  return (unsigned long long)__double2ll_rn((double)v * scale);
}
__device__ __forceinline__ void fix_add(long long* p, float v, double scale) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), fix_quantize(v, scale));
}
__device__ __forceinline__ float fix_to_float(long long acc, double inv) { return (float)((double)acc * inv); }  // inv: 2^-shift
