// Picture artefacts for gfx950: the 8-bit RGB conversions behind `--save_png`, one launch per picture.
//
// Replaces (reference paths):
//   colorplot_light + get_Middlebury_colorwheel     flow_library/flow_plot.py:56-105,157-203
//   save_image's scaling + quickvis_tensor's cast   helper_functions/logging.py:307-315, ownutilities.py:413-415
//   maximum_flow, max |delta|                       helper_functions/ownutilities.py:379-389, attack_PCFA.py:273-274
//
// Inputs are [B,C,H,W] fp32 views (four element strides, as pcfa_avg_epe takes them); outputs are dense uint8 [B,H,W,3].
// Every scale (a flow's longest vector, the perturbations' common maximum) is read from device memory, so a pair's ten
// pictures are ten launches with no host read in between.  The output is one flat run of B*H*W pixels: a thread converts four
// consecutive pixels and stores three whole dwords (the base is a tensor allocation, so dword 3t is aligned); the last
// (B*H*W) mod 4 pixels go out by bytes.  A group of four may straddle two rows or two items, so item and scale are looked
// up per pixel.  The maxima are exact whatever the order of reduction, hence reproducible: workgroup maxima meet in one
// vector atomic max on the bit pattern (non-negative floats order as unsigned integers).
#include "common.hpp"

namespace {

constexpr int ART_THREADS = 256;
constexpr int ART_MAX_BLOCKS = 2048;   // per item (maxima) resp. per launch (conversions): grid-stride beyond
constexpr int NCOLS = 55;              // RY 15 + YG 6 + GC 4 + CB 11 + BM 13 + MR 6

// The Middlebury colour wheel (Baker et al., "A Database and Evaluation Methodology for Optical Flow", ICCV 2007): six
// segments between the primary and secondary colours, one channel ramping by floor(255 * i / n) inside each.
struct Wheel {
  unsigned char c[NCOLS][3];
};
constexpr Wheel make_wheel() {
  Wheel w{};
  const int seg[6] = {15, 6, 4, 11, 13, 6};
  // per segment: the channel held at 255, the channel that ramps, and whether it ramps up (0 -> 255) or down
  const int full[6] = {0, 1, 1, 2, 2, 0};
  const int ramp[6] = {1, 0, 2, 1, 0, 2};
  const bool up[6] = {true, false, true, false, true, false};
  int col = 0;
  for (int s = 0; s < 6; ++s)
    for (int i = 0; i < seg[s]; ++i, ++col) {
      const int r = (255 * i) / seg[s];
      w.c[col][0] = w.c[col][1] = w.c[col][2] = 0;
      w.c[col][full[s]] = 255;
      w.c[col][ramp[s]] = (unsigned char)(up[s] ? r : 255 - r);
    }
  return w;
}
__constant__ Wheel g_wheel = make_wheel();

struct View4 {
  long long sb, sc, sh, sw;
};
inline View4 mkview(const long long s[4]) { return View4{s[0], s[1], s[2], s[3]}; }

// One correctly rounded fp32 operation each, never fused with a neighbour.  hipcc's __fadd_rn / __fmul_rn are the plain
// operators, which it contracts into an fma where it can, and its __fsqrt_rn is the approximate native root; the pragma
// takes the `contract` flag off the operation itself, so it survives inlining, and sqrtf / `/` are the correctly rounded
// forms under this library's flags (no fast-math).
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return __fadd_rn(a, b);
}
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return __fmul_rn(a, b);
}
__device__ __forceinline__ float div_rn(float a, float b) {
#pragma clang fp contract(off)
  return a / b;
}

// truncation toward zero, saturated: NaN and negatives -> 0, above 255 -> 255
__device__ __forceinline__ unsigned sat_u8(float v) {
  return (unsigned)fminf(fmaxf(v, 0.f), 255.f);   // fmaxf(NaN, 0) = 0
}

// ---------------------------------------------------------------- maxima
__global__ void zero_items_kernel(float* __restrict__ out, int items) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < items) out[i] = 0.f;
}

__global__ __launch_bounds__(ART_THREADS) void flow_maxlen_kernel(const float* __restrict__ flow, View4 fs, int H, int W,
                                                                   float* __restrict__ out) {
  __shared__ float red[4];
  const long long npix = (long long)H * W;
  const long long step = (long long)gridDim.x * blockDim.x;
  const float* f = flow + (long long)blockIdx.y * fs.sb;
  float m = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += step) {
    const long long y = i / W, x = i - y * W;
    const long long o = y * fs.sh + x * fs.sw;
    const float u = f[o], v = f[o + fs.sc];
    // one rounding per operation, as numpy's sqrt(u*u + v*v); a NaN component counts as length 0
    const float len = sqrtf(add_rn(mul_rn(u, u), mul_rn(v, v)));
    if (u == u && v == v) m = fmaxf(m, len);
  }
  m = block_max_256(m, red);
  if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned*>(out) + blockIdx.y, __float_as_uint(m));
}

__global__ __launch_bounds__(ART_THREADS) void absmax_kernel(const float* __restrict__ x, long long n,
                                                              float* __restrict__ out) {
  __shared__ float red[4];
  const long long step = (long long)gridDim.x * blockDim.x;
  const float* p = x + (long long)blockIdx.y * n;
  float m = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) m = fmaxf(m, fabsf(p[i]));
  m = block_max_256(m, red);
  if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned*>(out) + blockIdx.y, __float_as_uint(m));
}

// ---------------------------------------------------------------- per-pixel conversions
struct FlowColour {
  const float* flow;
  View4 fs;
  const float* scale;   // [items]

  // colorplot_light for one pixel -> r | g << 8 | b << 16
  __device__ __forceinline__ unsigned operator()(long long b, long long y, long long x) const {
    const long long o = b * fs.sb + y * fs.sh + x * fs.sw;
    float u = flow[o], v = flow[o + fs.sc];
    if (!(u == u && v == v)) return 0u;
    const float s = scale[b] + 1e-5f;
    u = u / s;
    v = v / s;
    const float rad = sqrtf(u * u + v * v);
    const float a = atan2f(-v, -u) / 3.14159265358979323846f;
    const float fk = (a + 1.f) / 2.f * (float)(NCOLS - 1);
    int k0 = (int)floorf(fk);
    k0 = min(max(k0, 0), NCOLS - 1);   // fk lies in [0, 54]; the clamp only keeps a stray rounding inside the table
    const int k1 = k0 + 1 == NCOLS ? 0 : k0 + 1;
    const float f = fk - (float)k0;
    unsigned rgb = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float c0 = (float)g_wheel.c[k0][c] / 255.f, c1 = (float)g_wheel.c[k1][c] / 255.f;
      float col = (1.f - f) * c0 + f * c1;
      col = rad <= 1.f ? 1.f - rad * (1.f - col) : col * 0.75f;
      rgb |= sat_u8(floorf(255.f * col)) << (8 * c);
    }
    return rgb;
  }
};

struct ImageU8 {
  const float* x;
  View4 xs;
  const float* add;   // or null
  View4 as;
  const float* m;     // or null; item b reads m[b * m_stride]
  long long m_stride;
  float gain;         // 255 for unit-range input, 1 for input that is in levels already (x * 1 is x)

  __device__ __forceinline__ unsigned operator()(long long b, long long y, long long px) const {
    const long long o = b * xs.sb + y * xs.sh + px * xs.sw;
    const long long oa = b * as.sb + y * as.sh + px * as.sw;
    const float mb = m ? m[b * m_stride] : 1.f;
    unsigned rgb = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = x[o + c * xs.sc];
      // one rounding per operation and no contraction: the bits of fp32 (x + d) * 255
      if (add) v = add_rn(v, add[oa + c * as.sc]);
      if (m) v = add_rn(mul_rn(div_rn(v, mb), 0.5f), 0.5f);
      rgb |= sat_u8(mul_rn(v, gain)) << (8 * c);
    }
    return rgb;
  }
};

template <typename Pixel>
__global__ __launch_bounds__(ART_THREADS) void rgb8_kernel(Pixel px, int H, int W, long long total,
                                                            unsigned char* __restrict__ out) {
  const long long hw = (long long)H * W;
  const long long groups = (total + 3) / 4;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += step) {
    const long long p0 = g * 4;
    const int n = total - p0 < 4 ? (int)(total - p0) : 4;
    unsigned rgb[4] = {0u, 0u, 0u, 0u};
    for (int k = 0; k < n; ++k) {
      const long long p = p0 + k;
      const long long b = p / hw, r = p - b * hw;
      const long long y = r / W, x = r - y * W;
      rgb[k] = px(b, y, x);
    }
    if (n == 4) {   // twelve bytes = three whole dwords at byte 12 g
      unsigned* o = reinterpret_cast<unsigned*>(out) + g * 3;
      o[0] = rgb[0] | (rgb[1] << 24);
      o[1] = (rgb[1] >> 8) | (rgb[2] << 16);
      o[2] = (rgb[2] >> 16) | (rgb[3] << 8);
    } else {
      for (int k = 0; k < n; ++k) {
        unsigned char* o = out + (p0 + k) * 3;
        o[0] = (unsigned char)(rgb[k] & 0xff);
        o[1] = (unsigned char)((rgb[k] >> 8) & 0xff);
        o[2] = (unsigned char)(rgb[k] >> 16);
      }
    }
  }
}

inline int max_blocks(long long work) {
  const long long b = (work + ART_THREADS - 1) / ART_THREADS;
  return (int)(b < ART_MAX_BLOCKS ? b : ART_MAX_BLOCKS);
}

inline bool bad_items(int items) { return items < 1 || items > 65535; }   // items ride on the grid's y axis

}  // namespace

extern "C" int pcfa_flow_maxlen_items(const float* flow, const long long strides[4], int items, int H, int W, float* out,
                                      void* stream) {
  if (!flow || !strides || !out || bad_items(items) || H < 1 || W < 1) return PCFA_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  pcfa_launch(zero_items_kernel, dim3(pcfa_cdiv(items, ART_THREADS)), dim3(ART_THREADS), 0, s, out, items);
  PCFA_LAUNCH_CHECK();
  pcfa_launch(flow_maxlen_kernel, dim3(max_blocks((long long)H * W), items), dim3(ART_THREADS), 0, s, flow, mkview(strides),
              H, W, out);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" int pcfa_absmax_items(const float* x, int items, long long n, float* out, void* stream) {
  if (!x || !out || bad_items(items) || n < 1) return PCFA_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  pcfa_launch(zero_items_kernel, dim3(pcfa_cdiv(items, ART_THREADS)), dim3(ART_THREADS), 0, s, out, items);
  PCFA_LAUNCH_CHECK();
  pcfa_launch(absmax_kernel, dim3(max_blocks(n), items), dim3(ART_THREADS), 0, s, x, n, out);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" int pcfa_flow_colour_u8(const float* flow, const long long strides[4], const float* scale, int items, int H,
                                   int W, unsigned char* out, void* stream) {
  if (!flow || !strides || !scale || !out || items < 1 || H < 1 || W < 1) return PCFA_ERR_INVALID_ARG;
  const long long total = (long long)items * H * W;
  pcfa_launch(rgb8_kernel<FlowColour>, dim3(max_blocks((total + 3) / 4)), dim3(ART_THREADS), 0, (hipStream_t)stream,
              FlowColour{flow, mkview(strides), scale}, H, W, total, out);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" int pcfa_image_u8(const float* x, const long long strides[4], const float* add, const long long add_strides[4],
                             const float* m, long long m_stride, int unit_input, int items, int H, int W,
                             unsigned char* out, void* stream) {
  if (!x || !strides || !out || items < 1 || H < 1 || W < 1 || (add && !add_strides) || m_stride < 0)
    return PCFA_ERR_INVALID_ARG;
  const float gain = (unit_input || m) ? 255.f : 1.f;   // a normalised perturbation is unit-range whatever came in
  const long long total = (long long)items * H * W;
  const View4 as = add ? mkview(add_strides) : View4{0, 0, 0, 0};
  pcfa_launch(rgb8_kernel<ImageU8>, dim3(max_blocks((total + 3) / 4)), dim3(ART_THREADS), 0, (hipStream_t)stream,
              ImageU8{x, mkview(strides), add, as, m, m_stride, gain}, H, W, total, out);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}
