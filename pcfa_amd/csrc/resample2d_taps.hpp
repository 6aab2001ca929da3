// Resample2d's neighbour taps (reference resample2d_kernel.cu:44-62, :103-111), shared by the forward / atomic backward
// of flownet_ops.hip and the fixed-point backward of warp_ops.hip.
#pragma once
#include <hip/hip_runtime.h>

struct RsTaps {
  int xL, xR, yT, yB;
  float alpha, beta;
};

__device__ __forceinline__ RsTaps rs_taps(float xf, float yf, int h, int w) {
  RsTaps t;
  const float fx = floorf(xf), fy = floorf(yf);
  t.alpha = xf - fx;
  t.beta = yf - fy;
  t.xL = max(min((int)fx, w - 1), 0);
  t.xR = max(min((int)(fx + 1.f), w - 1), 0);
  t.yT = max(min((int)fy, h - 1), 0);
  t.yB = max(min((int)(fy + 1.f), h - 1), 0);
  return t;
}
