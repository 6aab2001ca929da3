// The output tail of the 3x3 convolutions, stated once for the four places that finish an output element: the epilogue of
// conv3x3_winograd_kernel (conv3x3.hip), the epilogue of conv3x3_f43_kernel<ACT, false> and f43_finish_kernel<ACT, 23 | 43>
// (conv3x3_f43.hip).  Which of them a layer lands on depends on its shape, so the order and the roundings below are one
// rule, not three.  No loads here: every site adds its own bias and hands in its mask / addend operands (below).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ACT: 0 none, 1 ReLU, 2 LeakyReLU(slope) as torch: x > 0 ? x : x * negative_slope
template <int ACT>
__device__ __forceinline__ float act_apply(float y, float slope) {
  if (ACT == 1) return fmaxf(y, 0.f);
  if (ACT == 2) return y > 0.f ? y : y * slope;
  return y;
}

// Data gradient w.r.t. a (Leaky)ReLU output m: the deferred activation backward of the producer, factor 1 where its
// output is positive, else the producer's slope ms.  ms == 0 (ReLU) SELECTS an exact zero; it is not a product.
__device__ __forceinline__ float deferred_mask(float v, float m, float ms) {
  return m > 0.f ? v : (ms == 0.f ? 0.f : v * ms);
}
__device__ __forceinline__ float4 deferred_mask(float4 v, float4 m, float ms) {
  return make_float4(deferred_mask(v.x, m.x, ms), deferred_mask(v.y, m.y, ms), deferred_mask(v.z, m.z, ms),
                     deferred_mask(v.w, m.w, ms));
}

// The ordered tail of four output values of one channel.  y = pre-activation with the bias added.  mask_all: the mask
// covers these elements and comes BEFORE the addend; mask_prefix: they lie in the masked channel prefix (mask_channels
// > 0), whose mask comes AFTER the addend (the dense-block backward: the gradient is complete only with the other
// consumer's share).  Data gradients run with ACT = 0 and `slope` is then the mask's factor.
// m() / a() return the four mask / addend values and are called only where the rule uses them: a site that loads at the
// store address keeps the load inside the condition, one that fetched them earlier returns its registers.
template <int ACT, typename M, typename A>
__device__ __forceinline__ float4 conv_tail(float4 y, float slope, bool mask_all, bool mask_prefix, M&& m, bool has_addend,
                                            A&& a) {
  const float ms = ACT == 0 ? slope : 0.f;
  y = make_float4(act_apply<ACT>(y.x, slope), act_apply<ACT>(y.y, slope), act_apply<ACT>(y.z, slope),
                  act_apply<ACT>(y.w, slope));
  if (mask_all) y = deferred_mask(y, m(), ms);
  if (has_addend) {
    const float4 ad = a();
    y = make_float4(y.x + ad.x, y.y + ad.y, y.z + ad.z, y.w + ad.w);
  }
  if (mask_prefix) y = deferred_mask(y, m(), ms);
  return y;
}
