// Resample2d's neighbour taps (reference resample2d_kernel.cu:44-62, :103-111) and its per-pixel backward body, shared by
// the forward / atomic backward of flownet_ops.hip and the fixed-point backward of warp_ops.hip.
#pragma once
#include <hip/hip_runtime.h>

// floor -> tap index for ANY float: (int) of a value outside int's range, or of NaN, is undefined, so the floor is clamped
// to +-1e8 before the conversion (fmaxf / fminf return the other operand for NaN: NaN -> -1e8), as make_origin of the
// correlation lookups does.  Every index, window cell and difference formed from the result stays far inside int; for a
// floor within +-1e8 -- any image -- the value is the plain conversion's.
__device__ __forceinline__ int tap_index(float f) { return (int)fminf(fmaxf(f, -1.0e8f), 1.0e8f); }

struct RsTaps {
  int xL, xR, yT, yB;
  float alpha, beta;
};

__device__ __forceinline__ RsTaps rs_taps(float xf, float yf, int h, int w) {
  RsTaps t;
  const float fx = floorf(xf), fy = floorf(yf);
  t.alpha = xf - fx;
  t.beta = yf - fy;
  t.xL = max(min(tap_index(fx), w - 1), 0);
  t.xR = max(min(tap_index(fx + 1.f), w - 1), 0);
  t.yT = max(min(tap_index(fy), h - 1), 0);
  t.yB = max(min(tap_index(fy + 1.f), h - 1), 0);
  return t;
}

// One output pixel (idx over B x H x W) of Resample2d's backward (resample2d_kernel.cu:75-201), in1 of size iH x iW:
// put(element of grad_in1, addend) scatters grad_out, the flow gradient is the reference's gather, written directly (one
// thread owns every channel of its pixel).  The statement sequence restates the reference and is not to be tidied: both
// kernels (fp32 atomics / fixed point) must form the same addends and the same gdx / gdy chains.
template <class Put>
__device__ __forceinline__ void resample2d_bwd_pixel(const float* __restrict__ in1, const float* __restrict__ flow,
                                                     const float* __restrict__ gout, float* __restrict__ gflow, long long idx,
                                                     int C, int iH, int iW, int H, int W, Put put) {
  const int x = idx % W, y = (idx / W) % H, b = (int)(idx / ((long long)W * H));
  const size_t plane = (size_t)H * W, iplane = (size_t)iH * iW;
  const float dx = flow[((size_t)b * 2) * plane + (size_t)y * W + x];
  const float dy = flow[((size_t)b * 2 + 1) * plane + (size_t)y * W + x];
  const float xf = (float)x + dx, yf = (float)y + dy;
  // grad_in1: neighbours clamped against the INPUT size, weights from truncation (xf - int(xf), :103-111; truncf is
  // (float)(int) wherever that is defined)
  const RsTaps t1 = rs_taps(xf, yf, iH, iW);
  const float a1 = xf - truncf(xf), b1 = yf - truncf(yf);
  // grad_flow: neighbours clamped against the flow size, gamma = 1 - frac (:159-170)
  const RsTaps t2 = rs_taps(xf, yf, H, W);
  const float gam_x = 1.f - t2.alpha, gam_y = 1.f - t2.beta;
  const float* g = gout + (size_t)b * C * plane + (size_t)y * W + x;
  float gdx = 0.f, gdy = 0.f;
  for (int c = 0; c < C; ++c) {
    const float gv = g[(size_t)c * plane];
    const size_t d = ((size_t)b * C + c) * iplane;
    put(d + (size_t)t1.yT * iW + t1.xL, (1.f - a1) * (1.f - b1) * gv);
    put(d + (size_t)t1.yT * iW + t1.xR, a1 * (1.f - b1) * gv);
    put(d + (size_t)t1.yB * iW + t1.xL, (1.f - a1) * b1 * gv);
    put(d + (size_t)t1.yB * iW + t1.xR, a1 * b1 * gv);
    const float* s = in1 + d;
    const float iTL = s[(size_t)t2.yT * iW + t2.xL], iTR = s[(size_t)t2.yT * iW + t2.xR];
    const float iBL = s[(size_t)t2.yB * iW + t2.xL], iBR = s[(size_t)t2.yB * iW + t2.xR];
    // channel 0 (d/dx): gamma from the y fraction; channel 1 (d/dy): gamma from the x fraction
    gdx += gam_y * gv * iTR;
    gdx -= gam_y * gv * iTL;
    gdx += (1.f - gam_y) * gv * iBR;
    gdx -= (1.f - gam_y) * gv * iBL;
    gdy += gam_x * gv * iBL;
    gdy -= gam_x * gv * iTL;
    gdy += (1.f - gam_x) * gv * iBR;
    gdy -= (1.f - gam_x) * gv * iTR;
  }
  gflow[((size_t)b * 2) * plane + (size_t)y * W + x] = gdx;
  gflow[((size_t)b * 2 + 1) * plane + (size_t)y * W + x] = gdy;
}
