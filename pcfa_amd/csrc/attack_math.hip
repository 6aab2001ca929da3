// Fused attack math for gfx950: box-constraint transforms, perturbation
// extraction, and the PCFA loss (similarity term + L2 penalty) with its gradient.
//
// Replaces (reference paths):
//   ScaledInputModel.forward prologue   helper_functions/own_models.py:62-85
//   extract_deltas / extract_deltas_joint   attack_PCFA.py:20-37
//   avg_epe / avg_mse / f_cosim / relu_penalty / loss_delta_constraint
//                                        helper_functions/losses.py:3-44,76-88,110-126,177-230
//
// All kernels are HBM-streaming: 16-B vector loads where the layout allows,
// grid capped at 2048 workgroups with grid-stride loops.  Reductions are two
// stage (per-workgroup partials in a fixed slot, then one workgroup sums them in
// index order), so every scalar is bitwise reproducible run to run -- L-BFGS
// amplifies summation-order noise.
#include "common.hpp"

namespace {

constexpr int RED_BLOCKS = 1024;  // fixed: the partial count defines the summation order
constexpr int RED_THREADS = 256;
constexpr int NSUM = 8;           // partial sums per workgroup

struct BoxConst {
  float k;  // 0.5 / (1 - eps)   (evaluated in double like the Python scalar, then rounded)
  float c;  // 1 - eps
};
inline BoxConst make_box(double eps) {
  BoxConst b;
  b.k = (float)((1. / 2.) * 1. / (1. - eps));
  b.c = (float)(1. - eps);
  return b;
}

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// ---------------------------------------------------------------- box transform
__global__ void box_fwd_kernel(const float* __restrict__ image, const float* __restrict__ delta,
                               float* __restrict__ out, int B, long long n, int cov, BoxConst bc,
                               float scale) {
  const long long total = (long long)B * n;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    float x = image[i];
    if (delta) x = x + delta[i % n];
    if (cov) x = bc.k * (tanhf(x) + bc.c);
    x = clamp01(x);
    if (scale != 1.f) x = scale * x;
    out[i] = x;
  }
}

// grad wrt (image+delta); grad_delta is the batch sum in index order.
__global__ void box_bwd_kernel(const float* __restrict__ image, const float* __restrict__ delta,
                               const float* __restrict__ gout, float* __restrict__ gimage,
                               float* __restrict__ gdelta, int B, long long n, int cov,
                               BoxConst bc, float scale) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
    float gsum = 0.f;
    const float d = delta ? delta[j] : 0.f;
    for (int b = 0; b < B; ++b) {
      const long long i = (long long)b * n + j;
      float x = image[i];
      if (delta) x = x + d;
      float g = gout[i];
      if (scale != 1.f) g = g * scale;
      float y = x, t = 0.f;
      if (cov) {
        t = tanhf(x);
        y = bc.k * (t + bc.c);
      }
      if (!(y >= 0.f && y <= 1.f)) g = 0.f;  // clamp backward: pass-through inside [0,1]
      if (cov) g = (g * bc.k) * (1.f - t * t);
      if (gimage) gimage[i] = g;
      gsum += g;
    }
    if (gdelta) gdelta[j] = gsum;
  }
}

// ---------------------------------------------------------------- extract_deltas
__global__ void deltas_fwd_kernel(const float* __restrict__ w, const float* __restrict__ image,
                                  float* __restrict__ delta, long long n, int cov, BoxConst bc) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float x = w[i];
    const float y = cov ? bc.k * (tanhf(x) + bc.c) : clamp01(x);
    delta[i] = y - image[i];
  }
}

__global__ void deltas_bwd_kernel(const float* __restrict__ w, const float* __restrict__ gd,
                                  float* __restrict__ gw, long long n, int cov, BoxConst bc) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float x = w[i];
    float g = gd[i];
    if (cov) {
      const float t = tanhf(x);
      g = (g * bc.k) * (1.f - t * t);
    } else if (!(x >= 0.f && x <= 1.f)) {
      g = 0.f;
    }
    gw[i] = g;
  }
}

__global__ void deltas_joint_fwd_kernel(const float* __restrict__ nd,
                                        const float* __restrict__ imax,
                                        const float* __restrict__ imin, float* __restrict__ delta,
                                        long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float up = clamp01(nd[i] + imax[i]) - imax[i];
    delta[i] = clamp01(up + imin[i]) - imin[i];
  }
}

__global__ void deltas_joint_bwd_kernel(const float* __restrict__ nd,
                                        const float* __restrict__ imax,
                                        const float* __restrict__ imin,
                                        const float* __restrict__ gd, float* __restrict__ gnd,
                                        long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float a = nd[i] + imax[i];
    const float up = clamp01(a) - imax[i];
    const float b = up + imin[i];
    float g = gd[i];
    if (!(b >= 0.f && b <= 1.f)) g = 0.f;
    if (!(a >= 0.f && a <= 1.f)) g = 0.f;
    gnd[i] = g;
  }
}

// ---------------------------------------------------------------- reductions
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// Sum NS values over the workgroup; result valid in thread 0.
template <int NS>
__device__ __forceinline__ void block_sum(float (&v)[NS], float* smem /*[NS][4]*/) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const float s = wave_sum(v[k]);
    if (lane == 0) smem[k * 4 + wave] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NS; ++k)
      v[k] = ((smem[k * 4 + 0] + smem[k * 4 + 1]) + smem[k * 4 + 2]) + smem[k * 4 + 3];
  }
}

struct View4 {
  long long sb, sc, sh, sw;
};

// The *_items entry points put item b = blockIdx.y of a batch of independent attacks on the grid's y axis: every base
// pointer moves by its item stride (in floats) and the item then runs the very blocks, threads and summation order of the
// single call on its slice -- which is a launch with gridDim.y == 1 and all strides unused.
struct LossItemStride {
  long long pred, target, d1, d2;
};

// partial[block][0]=sum epe, [1]=sum sq diff, [2]=p.t, [3]=p.p, [4]=t.t, [5]=sum d1^2, [6]=sum d2^2
__global__ __launch_bounds__(RED_THREADS) void loss_partial_kernel(
    const float* __restrict__ pred, View4 ps, const float* __restrict__ target, View4 ts, int B,
    int H, int W, const float* __restrict__ d1, long long n1, const float* __restrict__ d2,
    long long n2, float* __restrict__ partial, LossItemStride is) {
  __shared__ float smem[NSUM * 4];
  float v[NSUM];
#pragma unroll
  for (int k = 0; k < NSUM; ++k) v[k] = 0.f;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long item = blockIdx.y;
  partial += item * gridDim.x * NSUM;
  if (pred) {
    pred += item * is.pred;
    target += item * is.target;
    const long long npix = (long long)B * H * W;
    for (long long i = gid; i < npix; i += stride) {
      const int x = i % W;
      const long long t = i / W;
      const int y = t % H;
      const int b = (int)(t / H);
      const long long po = b * ps.sb + y * ps.sh + x * ps.sw;
      const long long to = b * ts.sb + y * ts.sh + x * ts.sw;
      const float pu = pred[po], pv = pred[po + ps.sc];
      const float tu = target[to], tv = target[to + ts.sc];
      const float du = pu - tu, dv = pv - tv;
      const float sq = du * du + dv * dv;
      v[0] += sqrtf(sq);
      v[1] += sq;
      v[2] += pu * tu + pv * tv;
      v[3] += pu * pu + pv * pv;
      v[4] += tu * tu + tv * tv;
    }
  }
  if (d1) {
    d1 += item * is.d1;
    for (long long i = gid; i < n1; i += stride) v[5] += d1[i] * d1[i];
  }
  if (d2) {
    d2 += item * is.d2;
    for (long long i = gid; i < n2; i += stride) v[6] += d2[i] * d2[i];
  }
  block_sum<NSUM>(v, smem);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NSUM; ++k) partial[(size_t)blockIdx.x * NSUM + k] = v[k];
  }
}

// mode 0: loss_delta_constraint scalars; mode 1: avg_epe only; mode 2: sum of squares (slot 5).
// Item blockIdx.y reads its own partials and writes out[item * out_stride ...].
__global__ __launch_bounds__(RED_THREADS) void loss_final_kernel(
    const float* __restrict__ partial, int nblocks, float* __restrict__ out, int mode,
    float npix, float nelem_flow, float ndelta, float bound_sq, float mu, int f_type, int out_stride) {
  __shared__ float smem[NSUM * 4];
  float v[NSUM];
#pragma unroll
  for (int k = 0; k < NSUM; ++k) v[k] = 0.f;
  partial += (size_t)blockIdx.y * nblocks * NSUM;
  out += (size_t)blockIdx.y * out_stride;
  for (int i = threadIdx.x; i < nblocks; i += blockDim.x) {
#pragma unroll
    for (int k = 0; k < NSUM; ++k) v[k] += partial[(size_t)i * NSUM + k];
  }
  block_sum<NSUM>(v, smem);
  if (threadIdx.x != 0) return;
  if (mode == 1) {
    out[0] = v[0] / npix;
    return;
  }
  if (mode == 2) {
    out[0] = v[5];
    return;
  }
  float sim;
  if (f_type == PCFA_LOSS_AEE)
    sim = v[0] / npix;
  else if (f_type == PCFA_LOSS_MSE)
    sim = v[1] / nelem_flow;
  else  // bug-compatible with losses.py:88:  1 - (p.t / sqrt(p.p)) * sqrt(t.t)
    sim = 1.f - v[2] / sqrtf(v[3]) * sqrtf(v[4]);
  const float msq = (v[5] + v[6]) / ndelta;
  const float pen = fmaxf(0.f, msq - bound_sq);
  out[0] = sim + mu * pen;
  out[1] = sim;
  out[2] = msq;
  out[3] = v[2];
  out[4] = v[3];
  out[5] = v[4];
  out[6] = msq - bound_sq;
}

// total = ((L_0 + L_1) + ...) + L_{items-1}: the in-order fp32 sum of the items' losses
__global__ void loss_items_total_kernel(const float* __restrict__ scal, int items, float* __restrict__ total) {
  float s = scal[0];
  for (int b = 1; b < items; ++b) s += scal[(size_t)b * 8];
  total[0] = s;
}

__global__ void loss_bwd_flow_kernel(const float* __restrict__ pred, View4 ps,
                                     const float* __restrict__ target, View4 ts, int B, int H,
                                     int W, int f_type, const float* __restrict__ fwd,
                                     const float* __restrict__ gloss, float* __restrict__ gpred,
                                     LossItemStride is) {
  const long long npix = (long long)B * H * W;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long item = blockIdx.y;
  pred += item * is.pred;
  target += item * is.target;
  fwd += item * 8;
  gpred += item * 2 * npix;
  const float gl = gloss[0];
  const float pt = fwd[3], pp = fwd[4], tt = fwd[5];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += stride) {
    const int x = i % W;
    const long long t = i / W;
    const int y = t % H;
    const int b = (int)(t / H);
    const long long po = b * ps.sb + y * ps.sh + x * ps.sw;
    const long long to = b * ts.sb + y * ts.sh + x * ts.sw;
    const float pu = pred[po], pv = pred[po + ps.sc];
    const float tu = target[to], tv = target[to + ts.sc];
    float gu, gv;
    if (f_type == PCFA_LOSS_AEE) {
      // mean -> sqrt -> sum(dim=1) -> pow(2) -> sub, in autograd's order
      const float du = pu - tu, dv = pv - tv;
      const float g = gl / (float)npix;
      const float gs = g / (2.f * sqrtf(du * du + dv * dv));
      gu = gs * (2.f * du);
      gv = gs * (2.f * dv);
    } else if (f_type == PCFA_LOSS_MSE) {
      const float g = gl / (float)(npix * 2);
      gu = g * (2.f * (pu - tu));
      gv = g * (2.f * (pv - tv));
    } else {
      const float spp = sqrtf(pp), stt = sqrtf(tt);
      // L = 1 - pt * pp^-1/2 * tt^1/2
      const float a = -gl * stt / spp;             // d/d(pt)
      const float c = gl * stt * pt / (2.f * pp * spp);  // d/d(pp)
      gu = a * tu + c * (2.f * pu);
      gv = a * tv + c * (2.f * pv);
    }
    const long long o = ((long long)b * 2 * H + y) * W + x;
    gpred[o] = gu;
    gpred[o + (long long)H * W] = gv;
  }
}

__global__ void loss_bwd_delta_kernel(const float* __restrict__ d, long long n, float ndelta,
                                      float mu, float mult, const float* __restrict__ fwd,
                                      const float* __restrict__ gloss, float* __restrict__ gd,
                                      long long item_stride) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  d += blockIdx.y * item_stride;
  gd += blockIdx.y * item_stride;
  fwd += blockIdx.y * 8;
  const float arg = fwd[6];  // msq - bound^2
  // torch.max(0, x) backward: full gradient for x > 0, half at the tie, none below
  const float sel = arg > 0.f ? 1.f : (arg == 0.f ? 0.5f : 0.f);
  const float g = gloss[0] * mu * sel / ndelta;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    gd[i] = mult * (g * (2.f * d[i]));
}

inline int ew_blocks(long long n) {
  long long b = (n + 255) / 256;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (int)b;
}

inline View4 mkview(const long long s[4]) { return View4{s[0], s[1], s[2], s[3]}; }

__global__ void null_kernel() {}

// Fills the workgroup's whole LDS allocation with `pattern` and lingers a little, so that the grid spreads over every CU.
__global__ __launch_bounds__(256) void poison_lds_kernel(unsigned pattern, int nwords) {
  extern __shared__ unsigned lds_words[];
  for (int i = threadIdx.x; i < nwords; i += 256) lds_words[i] = pattern;
  __syncthreads();
  for (int i = 0; i < 64; ++i) __builtin_amdgcn_s_sleep(32);
  // (a read the compiler cannot drop, so the stores above are kept)
  if (lds_words[(threadIdx.x * 97) % nwords] != pattern) __builtin_trap();
}

// The control of poison_lds_kernel: every workgroup reports word `blockIdx.x` of an LDS array it never wrote.
__global__ __launch_bounds__(64) void peek_lds_kernel(unsigned* __restrict__ out, int nwords) {
  extern __shared__ unsigned lds_words[];
  if (threadIdx.x == 0) {
    // (volatile: an uninitialised read the optimiser may not fold away)
    out[blockIdx.x] = reinterpret_cast<volatile unsigned*>(lds_words)[(blockIdx.x * 61) % nwords];
  }
}

}  // namespace

extern "C" int pcfa_abi_version(void) { return PCFA_ABI_VERSION; }

PcfaTimingState& pcfa_timing_state() {
  static thread_local PcfaTimingState state;
  return state;
}

extern "C" int pcfa_timing_arm(void* start_event, void* stop_event, int nth) {
  PcfaTimingState& t = pcfa_timing_state();
  if (nth < 0) {  // disarm: drop whatever is still queued
    t.n = 0;
    return PCFA_OK;
  }
  if (t.n >= 8) return PCFA_ERR_INVALID_ARG;
  if (t.n == 0) t.launched = 0;  // nth counts this thread's launches from the first arm of a batch
  t.q[t.n++] = PcfaArmed{(hipEvent_t)start_event, (hipEvent_t)stop_event, nth};
  return PCFA_OK;
}

// ---- calibration kernels (bench.py `calibration`): what the chip sustains on THIS box, next to the data-sheet peaks --------
namespace {
typedef float calib_f32x16 __attribute__((ext_vector_type(16)));

// Register-only v_mfma_f32_32x32x2_f32 loop: four independent accumulators per wave, operands from registers, pseudo-random
// data (the matrix pipe's clock depends on what it multiplies).  4096 flop per MFMA.
__global__ __launch_bounds__(256) void calib_mfma_f32_kernel(float* __restrict__ out, int iters) {
  const unsigned seed = (blockIdx.x * 256u + threadIdx.x) * 2654435761u + 12345u;
  float a0 = (float)(seed & 0xffff) * (1.0f / 65536.f) - 0.5f, b0 = (float)((seed >> 16) & 0xffff) * (1.0f / 65536.f) - 0.5f;
  float a1 = b0 * 0.75f + 0.1f, b1 = a0 * 0.5f - 0.2f;
  calib_f32x16 c0, c1, c2, c3;
#pragma unroll
  for (int r = 0; r < 16; ++r) c0[r] = c1[r] = c2[r] = c3[r] = 0.f;
  for (int i = 0; i < iters; ++i) {
    c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, c1, 0, 0, 0);
    c2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, c2, 0, 0, 0);
    c3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, c3, 0, 0, 0);
  }
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) s += c0[r] + c1[r] + c2[r] + c3[r];
  if (s == 123456.789f) out[0] = s;   // keeps the loop alive; never true in practice
}

__global__ __launch_bounds__(256) void calib_copy_kernel(const float4* __restrict__ src, float4* __restrict__ dst, long long n4) {
  const long long step = (long long)gridDim.x * blockDim.x;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * step < n4; i += 4 * step) {   // four 16-B loads in flight per lane
    const float4 a = src[i], b = src[i + step], c = src[i + 2 * step], d = src[i + 3 * step];
    dst[i] = a;
    dst[i + step] = b;
    dst[i + 2 * step] = c;
    dst[i + 3 * step] = d;
  }
  for (; i < n4; i += step) dst[i] = src[i];
}
}  // namespace

extern "C" long long pcfa_calib_mfma_f32(float* scratch, int blocks, int iters, void* stream) {
  if (!scratch || blocks < 1 || iters < 1) return -1;
  pcfa_launch(calib_mfma_f32_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, scratch, iters);
  if (hipGetLastError() != hipSuccess) return -1;
  return (long long)blocks * 4 * iters * 4 * 4096;   // waves x iterations x MFMAs x flop
}

extern "C" int pcfa_calib_copy(const float* src, float* dst, long long n_floats, void* stream) {
  if (!src || !dst || n_floats < 4 || n_floats % 4 != 0 || (reinterpret_cast<uintptr_t>(src) & 15) ||
      (reinterpret_cast<uintptr_t>(dst) & 15))
    return PCFA_ERR_INVALID_ARG;
  pcfa_launch(calib_copy_kernel, dim3(256 * 8), dim3(256), 0, (hipStream_t)stream, (const float4*)src, (float4*)dst,
              n_floats / 4);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" int pcfa_null_launch(void* stream) {
  pcfa_launch(null_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" int pcfa_poison_lds(unsigned pattern, void* stream) {
  constexpr int BYTES = 160 * 1024;   // the whole LDS of a CU: one workgroup per CU at a time, 8 rounds of 256
  static const hipError_t attr =
      hipFuncSetAttribute(reinterpret_cast<const void*>(poison_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, BYTES);
  if (attr != hipSuccess) return PCFA_ERR_UNSUPPORTED;
  pcfa_launch(poison_lds_kernel, dim3(2048), dim3(256), BYTES, (hipStream_t)stream, pattern, BYTES / 4);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" int pcfa_peek_lds(unsigned* out, int n, void* stream) {
  if (!out || n < 1 || n > 65535) return PCFA_ERR_INVALID_ARG;
  pcfa_launch(peek_lds_kernel, dim3((unsigned)n), dim3(64), 32 * 1024, (hipStream_t)stream, out, 32 * 1024 / 4);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" const char* pcfa_status_string(int status) {
  switch (status) {
    case PCFA_OK: return "ok";
    case PCFA_ERR_INVALID_ARG: return "invalid argument";
    case PCFA_ERR_UNSUPPORTED: return "unsupported parameter combination";
    case PCFA_ERR_WORKSPACE: return "workspace too small";
    default: return status > 0 ? hipGetErrorString((hipError_t)status) : "unknown status";
  }
}

extern "C" int pcfa_box_transform_fwd(const float* image, const float* delta, float* out, int B,
                                      long long n, int cov, double eps_box, float scale,
                                      void* stream) {
  if (!image || !out || B < 1 || n < 1) return PCFA_ERR_INVALID_ARG;
  pcfa_launch(box_fwd_kernel, dim3(ew_blocks((long long)B * n)), dim3(256), 0,
                     (hipStream_t)stream, image, delta, out, B, n, cov, make_box(eps_box), scale);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" int pcfa_box_transform_bwd(const float* image, const float* delta,
                                      const float* grad_out, float* grad_image, float* grad_delta,
                                      int B, long long n, int cov, double eps_box, float scale,
                                      void* stream) {
  if (!image || !grad_out || B < 1 || n < 1) return PCFA_ERR_INVALID_ARG;
  pcfa_launch(box_bwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, image,
                     delta, grad_out, grad_image, grad_delta, B, n, cov, make_box(eps_box), scale);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

// RAFT.forward / RAFTGMA.forward normalise both images with `2 * (image / 255.0) - 1.0` (models/raft/raft.py:88-89,
// models/gma/network.py:79-80): three elementwise launches per image, two more each in the backward and the gradient sums
// of image 1 (feature AND context encoder read it).  One launch per direction instead: pair = [n(image1); n(image2)]
// for the feature encoder, ctx = n(image1) once more for the context encoder.  Same fp32 operations in the same order
// as the three torch kernels on the GPU (a tensor divided by a host scalar is multiplied by the rounded reciprocal
// there), so the result is bit-identical.
__global__ void pm1_pair_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ pair,
                                    float* __restrict__ ctx, long long n, int B) {
  const float inv = 1.0f / 255.0f;
  const long long nb = (long long)n * B;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nb; i += (long long)gridDim.x * blockDim.x) {
    const float ya = 2.0f * (a[i] * inv) - 1.0f, yb = 2.0f * (b[i] * inv) - 1.0f;
    pair[i] = ya;
    pair[nb + i] = yb;
    ctx[i] = ya;
  }
}

__global__ void pm1_pair_bwd_kernel(const float* __restrict__ gpair, const float* __restrict__ gctx, float* __restrict__ ga,
                                    float* __restrict__ gb, long long n, int B) {
  const float inv = 1.0f / 255.0f;
  const long long nb = (long long)n * B;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nb; i += (long long)gridDim.x * blockDim.x) {
    const float g1 = gctx != nullptr ? gpair[i] + gctx[i] : gpair[i];   // autograd's sum of the two uses of n(image1)
    ga[i] = (g1 * 2.0f) * inv;
    gb[i] = (gpair[nb + i] * 2.0f) * inv;
  }
}

extern "C" int pcfa_pm1_pair_fwd(const float* image1, const float* image2, float* pair, float* ctx, int B, long long n,
                                 void* stream) {
  if (!image1 || !image2 || !pair || !ctx || B < 1 || n < 1) return PCFA_ERR_INVALID_ARG;
  pcfa_launch(pm1_pair_fwd_kernel, dim3(ew_blocks((long long)B * n)), dim3(256), 0, (hipStream_t)stream, image1, image2,
              pair, ctx, n, B);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" int pcfa_pm1_pair_bwd(const float* grad_pair, const float* grad_ctx, float* grad_image1, float* grad_image2,
                                 int B, long long n, void* stream) {
  if (!grad_pair || !grad_image1 || !grad_image2 || B < 1 || n < 1) return PCFA_ERR_INVALID_ARG;
  pcfa_launch(pm1_pair_bwd_kernel, dim3(ew_blocks((long long)B * n)), dim3(256), 0, (hipStream_t)stream, grad_pair,
              grad_ctx, grad_image1, grad_image2, n, B);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" int pcfa_extract_deltas_fwd(const float* nw_input, const float* image, float* delta,
                                       long long n, int cov, double eps_box, void* stream) {
  if (!nw_input || !image || !delta || n < 1) return PCFA_ERR_INVALID_ARG;
  pcfa_launch(deltas_fwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream,
                     nw_input, image, delta, n, cov, make_box(eps_box));
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" int pcfa_extract_deltas_bwd(const float* nw_input, const float* grad_delta,
                                       float* grad_nw_input, long long n, int cov, double eps_box,
                                       void* stream) {
  if (!nw_input || !grad_delta || !grad_nw_input || n < 1) return PCFA_ERR_INVALID_ARG;
  pcfa_launch(deltas_bwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream,
                     nw_input, grad_delta, grad_nw_input, n, cov, make_box(eps_box));
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" int pcfa_extract_deltas_joint_fwd(const float* nw_delta, const float* images_max,
                                             const float* images_min, float* delta, long long n,
                                             void* stream) {
  if (!nw_delta || !images_max || !images_min || !delta || n < 1) return PCFA_ERR_INVALID_ARG;
  pcfa_launch(deltas_joint_fwd_kernel, dim3(ew_blocks(n)), dim3(256), 0,
                     (hipStream_t)stream, nw_delta, images_max, images_min, delta, n);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" int pcfa_extract_deltas_joint_bwd(const float* nw_delta, const float* images_max,
                                             const float* images_min, const float* grad_delta,
                                             float* grad_nw_delta, long long n, void* stream) {
  if (!nw_delta || !images_max || !images_min || !grad_delta || !grad_nw_delta || n < 1)
    return PCFA_ERR_INVALID_ARG;
  pcfa_launch(deltas_joint_bwd_kernel, dim3(ew_blocks(n)), dim3(256), 0,
                     (hipStream_t)stream, nw_delta, images_max, images_min, grad_delta,
                     grad_nw_delta, n);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" size_t pcfa_flow_loss_workspace_bytes(void) {
  return sizeof(float) * RED_BLOCKS * NSUM;
}

extern "C" int pcfa_flow_loss_fwd(const float* pred, const long long pred_strides[4],
                                  const float* target, const long long target_strides[4], int B,
                                  int H, int W, const float* delta1, long long n1,
                                  const float* delta2, long long n2, float delta_bound, float mu,
                                  int f_type, float* out_scalars, void* workspace, void* stream) {
  if (!pred || !target || !pred_strides || !target_strides || !delta1 || !delta2 ||
      !out_scalars || !workspace || B < 1 || H < 1 || W < 1 || n1 < 1 || n2 < 1 || f_type < 0 ||
      f_type > 2)
    return PCFA_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  float* partial = (float*)workspace;
  pcfa_launch(loss_partial_kernel, dim3(RED_BLOCKS), dim3(RED_THREADS), 0, s, pred,
                     mkview(pred_strides), target, mkview(target_strides), B, H, W, delta1, n1,
                     delta2, n2, partial, LossItemStride{0, 0, 0, 0});
  PCFA_LAUNCH_CHECK();
  const float bound_sq = (float)((double)delta_bound * (double)delta_bound);
  pcfa_launch(loss_final_kernel, dim3(1), dim3(RED_THREADS), 0, s, partial, RED_BLOCKS,
                     out_scalars, 0, (float)((long long)B * H * W),
                     (float)((long long)B * 2 * H * W), (float)(n1 + n2), bound_sq, mu, f_type, 0);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" int pcfa_flow_loss_bwd(const float* pred, const long long pred_strides[4],
                                  const float* target, const long long target_strides[4], int B,
                                  int H, int W, const float* delta1, long long n1,
                                  const float* delta2, long long n2, float mu, int f_type,
                                  int joint, const float* fwd_scalars, const float* grad_loss,
                                  float* grad_pred, float* grad_delta1, float* grad_delta2,
                                  void* stream) {
  if (!pred || !target || !pred_strides || !target_strides || !fwd_scalars || !grad_loss ||
      B < 1 || H < 1 || W < 1 || f_type < 0 || f_type > 2)
    return PCFA_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (grad_pred) {
    pcfa_launch(loss_bwd_flow_kernel, dim3(ew_blocks((long long)B * H * W)), dim3(256), 0,
                       s, pred, mkview(pred_strides), target, mkview(target_strides), B, H, W,
                       f_type, fwd_scalars, grad_loss, grad_pred, LossItemStride{0, 0, 0, 0});
    PCFA_LAUNCH_CHECK();
  }
  const float ndelta = (float)(n1 + n2);
  if (grad_delta1) {
    if (!delta1) return PCFA_ERR_INVALID_ARG;
    pcfa_launch(loss_bwd_delta_kernel, dim3(ew_blocks(n1)), dim3(256), 0, s, delta1, n1,
                       ndelta, mu, joint ? 2.f : 1.f, fwd_scalars, grad_loss, grad_delta1, 0LL);
    PCFA_LAUNCH_CHECK();
  }
  if (grad_delta2) {
    if (!delta2) return PCFA_ERR_INVALID_ARG;
    pcfa_launch(loss_bwd_delta_kernel, dim3(ew_blocks(n2)), dim3(256), 0, s, delta2, n2,
                       ndelta, mu, 1.f, fwd_scalars, grad_loss, grad_delta2, 0LL);
    PCFA_LAUNCH_CHECK();
  }
  return PCFA_OK;
}

// ---------------------------------------------------------------- B independent attacks in one launch each
// Item b is the single call above with B = 1 on pred[b], target[b], delta1[b], delta2[b]: same grid x, same blocks, same
// order, hence the same bits.  delta1 / delta2 are dense [items][n1] / [items][n2]; a joint perturbation passes the same
// pointer twice.
namespace {
inline int items_status(int items) {
  if (items < 1) return PCFA_ERR_INVALID_ARG;
  if (items > PCFA_MAX_ITEMS) return PCFA_ERR_UNSUPPORTED;
  return PCFA_OK;
}
}  // namespace

extern "C" int pcfa_flow_loss_items_fwd(const float* pred, const long long pred_strides[4], const float* target,
                                        const long long target_strides[4], int items, int H, int W, const float* delta1,
                                        long long n1, const float* delta2, long long n2, float delta_bound, float mu,
                                        int f_type, float* out_scalars, float* out_total, void* workspace, void* stream) {
  if (!pred || !target || !pred_strides || !target_strides || !delta1 || !delta2 || !out_scalars || !out_total ||
      !workspace || H < 1 || W < 1 || n1 < 1 || n2 < 1 || f_type < 0 || f_type > 2)
    return PCFA_ERR_INVALID_ARG;
  if (int st = items_status(items)) return st;
  hipStream_t s = (hipStream_t)stream;
  float* partial = (float*)workspace;
  const LossItemStride is{pred_strides[0], target_strides[0], n1, n2};
  pcfa_launch(loss_partial_kernel, dim3(RED_BLOCKS, items), dim3(RED_THREADS), 0, s, pred, mkview(pred_strides), target,
              mkview(target_strides), 1, H, W, delta1, n1, delta2, n2, partial, is);
  PCFA_LAUNCH_CHECK();
  const float bound_sq = (float)((double)delta_bound * (double)delta_bound);
  pcfa_launch(loss_final_kernel, dim3(1, items), dim3(RED_THREADS), 0, s, partial, RED_BLOCKS, out_scalars, 0,
              (float)((long long)H * W), (float)((long long)2 * H * W), (float)(n1 + n2), bound_sq, mu, f_type, 8);
  PCFA_LAUNCH_CHECK();
  pcfa_launch(loss_items_total_kernel, dim3(1), dim3(1), 0, s, (const float*)out_scalars, items, out_total);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" int pcfa_flow_loss_items_bwd(const float* pred, const long long pred_strides[4], const float* target,
                                        const long long target_strides[4], int items, int H, int W, const float* delta1,
                                        long long n1, const float* delta2, long long n2, float mu, int f_type, int joint,
                                        const float* fwd_scalars, const float* grad_loss, float* grad_pred,
                                        float* grad_delta1, float* grad_delta2, void* stream) {
  if (!pred || !target || !pred_strides || !target_strides || !fwd_scalars || !grad_loss || H < 1 || W < 1 || n1 < 1 ||
      n2 < 1 || f_type < 0 || f_type > 2)
    return PCFA_ERR_INVALID_ARG;
  if (int st = items_status(items)) return st;
  hipStream_t s = (hipStream_t)stream;
  if (grad_pred) {
    const LossItemStride is{pred_strides[0], target_strides[0], 0, 0};
    pcfa_launch(loss_bwd_flow_kernel, dim3(ew_blocks((long long)H * W), items), dim3(256), 0, s, pred,
                mkview(pred_strides), target, mkview(target_strides), 1, H, W, f_type, fwd_scalars, grad_loss, grad_pred,
                is);
    PCFA_LAUNCH_CHECK();
  }
  const float ndelta = (float)(n1 + n2);
  if (grad_delta1) {
    if (!delta1) return PCFA_ERR_INVALID_ARG;
    pcfa_launch(loss_bwd_delta_kernel, dim3(ew_blocks(n1), items), dim3(256), 0, s, delta1, n1, ndelta, mu,
                joint ? 2.f : 1.f, fwd_scalars, grad_loss, grad_delta1, n1);
    PCFA_LAUNCH_CHECK();
  }
  if (grad_delta2) {
    if (!delta2) return PCFA_ERR_INVALID_ARG;
    pcfa_launch(loss_bwd_delta_kernel, dim3(ew_blocks(n2), items), dim3(256), 0, s, delta2, n2, ndelta, mu, 1.f,
                fwd_scalars, grad_loss, grad_delta2, n2);
    PCFA_LAUNCH_CHECK();
  }
  return PCFA_OK;
}

extern "C" int pcfa_avg_epe(const float* flow1, const long long strides1[4], const float* flow2,
                            const long long strides2[4], int B, int H, int W, float* out,
                            void* workspace, void* stream) {
  if (!flow1 || !flow2 || !strides1 || !strides2 || !out || !workspace || B < 1 || H < 1 ||
      W < 1)
    return PCFA_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  float* partial = (float*)workspace;
  pcfa_launch(loss_partial_kernel, dim3(RED_BLOCKS), dim3(RED_THREADS), 0, s, flow1,
                     mkview(strides1), flow2, mkview(strides2), B, H, W, (const float*)nullptr,
                     0LL, (const float*)nullptr, 0LL, partial, LossItemStride{0, 0, 0, 0});
  PCFA_LAUNCH_CHECK();
  pcfa_launch(loss_final_kernel, dim3(1), dim3(RED_THREADS), 0, s, partial, RED_BLOCKS,
                     out, 1, (float)((long long)B * H * W), 0.f, 1.f, 0.f, 0.f, 0, 0);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" int pcfa_avg_epe_items(const float* flow1, const long long strides1[4], const float* flow2,
                                  const long long strides2[4], int items, int H, int W, float* out, void* workspace,
                                  void* stream) {
  if (!flow1 || !flow2 || !strides1 || !strides2 || !out || !workspace || H < 1 || W < 1) return PCFA_ERR_INVALID_ARG;
  if (int st = items_status(items)) return st;
  hipStream_t s = (hipStream_t)stream;
  float* partial = (float*)workspace;
  pcfa_launch(loss_partial_kernel, dim3(RED_BLOCKS, items), dim3(RED_THREADS), 0, s, flow1, mkview(strides1), flow2,
              mkview(strides2), 1, H, W, (const float*)nullptr, 0LL, (const float*)nullptr, 0LL, partial,
              LossItemStride{strides1[0], strides2[0], 0, 0});
  PCFA_LAUNCH_CHECK();
  pcfa_launch(loss_final_kernel, dim3(1, items), dim3(RED_THREADS), 0, s, partial, RED_BLOCKS, out, 1,
              (float)((long long)H * W), 0.f, 1.f, 0.f, 0.f, 0, 1);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" int pcfa_sum_squares(const float* x, long long n, float* out, void* workspace,
                                void* stream) {
  if (!x || !out || !workspace || n < 1) return PCFA_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  float* partial = (float*)workspace;
  pcfa_launch(loss_partial_kernel, dim3(RED_BLOCKS), dim3(RED_THREADS), 0, s,
                     (const float*)nullptr, View4{0, 0, 0, 0}, (const float*)nullptr,
                     View4{0, 0, 0, 0}, 1, 1, 1, x, n, (const float*)nullptr, 0LL, partial,
                     LossItemStride{0, 0, 0, 0});
  PCFA_LAUNCH_CHECK();
  pcfa_launch(loss_final_kernel, dim3(1), dim3(RED_THREADS), 0, s, partial, RED_BLOCKS,
                     out, 2, 1.f, 1.f, 1.f, 0.f, 0.f, 0, 0);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" int pcfa_sum_squares_items(const float* x, int items, long long n, float* out, void* workspace,
                                      void* stream) {
  if (!x || !out || !workspace || n < 1) return PCFA_ERR_INVALID_ARG;
  if (int st = items_status(items)) return st;
  hipStream_t s = (hipStream_t)stream;
  float* partial = (float*)workspace;
  pcfa_launch(loss_partial_kernel, dim3(RED_BLOCKS, items), dim3(RED_THREADS), 0, s, (const float*)nullptr,
              View4{0, 0, 0, 0}, (const float*)nullptr, View4{0, 0, 0, 0}, 1, 1, 1, x, n, (const float*)nullptr, 0LL,
              partial, LossItemStride{0, 0, n, 0});
  PCFA_LAUNCH_CHECK();
  pcfa_launch(loss_final_kernel, dim3(1, items), dim3(RED_THREADS), 0, s, partial, RED_BLOCKS, out, 2, 1.f, 1.f, 1.f,
              0.f, 0.f, 0, 1);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

// ---------------------------------------------------------------- I-FGSM step (attack_FGSM.py:21-56, :208-209)
// One launch per iteration, in place: x_i <- clamp(x_i - epsilon * s_i, 0, 1), d_i = clamp(x_i, 0, 1) - img_i from the
// UPDATED x_i, with s_i = sign(g_i) (disjoint) or sign(0.5 * (g1 + g2)) for both images (joint).  Replaces the ~14 ATen
// element-wise launches of fgsm_attack_step(..., clipping=True) + clamp + subtract and reproduces them bit for bit: every
// operation below is ONE fp32 rounding in ATen's order (the explicit *_rn intrinsics keep the compiler from contracting or
// reassociating anything).
namespace {

constexpr int FGSM_THREADS = 256;
constexpr int FGSM_MAX_BLOCKS = 2048;

// torch.sign: -1, 0 or 1; 0 for +-0 and for NaN (both comparisons are false), +-1 for subnormals and +-inf
__device__ __forceinline__ float fgsm_sign(float g) { return (float)((0.f < g) - (g < 0.f)); }

// torch.clamp(v, 0, 1) on the GPU: NaN goes through, everything else through max then min (ATen's own expression, so a
// signed zero comes out as it does there); fminf / fmaxf alone would turn a NaN pixel into 0
__device__ __forceinline__ float fgsm_clamp01(float v) { return v != v ? v : fminf(fmaxf(v, 0.f), 1.f); }

__device__ __forceinline__ void fgsm_one(float x1, float x2, float g1, float g2, float i1, float i2, float eps, int joint,
                                         float& y1, float& y2, float& d1, float& d2) {
  float s1, s2;
  if (joint) {
    s1 = s2 = fgsm_sign(__fmul_rn(0.5f, __fadd_rn(g1, g2)));   // the sum is rounded (and may overflow) first
  } else {
    s1 = fgsm_sign(g1);
    s2 = fgsm_sign(g2);
  }
  y1 = fgsm_clamp01(__fsub_rn(x1, __fmul_rn(eps, s1)));
  y2 = fgsm_clamp01(__fsub_rn(x2, __fmul_rn(eps, s2)));
  d1 = __fsub_rn(fgsm_clamp01(y1), i1);   // (the second clamp is the identity on a clamped value, NaN included)
  d2 = __fsub_rn(fgsm_clamp01(y2), i2);
}

// VEC: every pointer is 16-byte aligned -> n / 4 float4 items grid-stride, then the n % 4 tail elements one per thread of
// the first workgroup.  !VEC: one float per thread and trip.
template <bool VEC>
__global__ __launch_bounds__(FGSM_THREADS) void fgsm_step_kernel(float* x1, float* x2, const float* __restrict__ g1,
                                                                 const float* __restrict__ g2,
                                                                 const float* __restrict__ img1,
                                                                 const float* __restrict__ img2, float* __restrict__ d1,
                                                                 float* __restrict__ d2, float eps, int joint, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long tail = 0;
  if (VEC) {
    const long long n4 = n >> 2;
    tail = n4 << 2;
    for (long long i = gid; i < n4; i += stride) {
      const float4 a1 = reinterpret_cast<const float4*>(x1)[i], a2 = reinterpret_cast<const float4*>(x2)[i];
      const float4 b1 = reinterpret_cast<const float4*>(g1)[i], b2 = reinterpret_cast<const float4*>(g2)[i];
      const float4 c1 = reinterpret_cast<const float4*>(img1)[i], c2 = reinterpret_cast<const float4*>(img2)[i];
      float4 y1, y2, e1, e2;
      fgsm_one(a1.x, a2.x, b1.x, b2.x, c1.x, c2.x, eps, joint, y1.x, y2.x, e1.x, e2.x);
      fgsm_one(a1.y, a2.y, b1.y, b2.y, c1.y, c2.y, eps, joint, y1.y, y2.y, e1.y, e2.y);
      fgsm_one(a1.z, a2.z, b1.z, b2.z, c1.z, c2.z, eps, joint, y1.z, y2.z, e1.z, e2.z);
      fgsm_one(a1.w, a2.w, b1.w, b2.w, c1.w, c2.w, eps, joint, y1.w, y2.w, e1.w, e2.w);
      reinterpret_cast<float4*>(x1)[i] = y1;
      reinterpret_cast<float4*>(x2)[i] = y2;
      reinterpret_cast<float4*>(d1)[i] = e1;
      reinterpret_cast<float4*>(d2)[i] = e2;
    }
  }
  for (long long i = tail + gid; i < n; i += stride) {
    float y1, y2, e1, e2;
    fgsm_one(x1[i], x2[i], g1[i], g2[i], img1[i], img2[i], eps, joint, y1, y2, e1, e2);
    x1[i] = y1;
    x2[i] = y2;
    d1[i] = e1;
    d2[i] = e2;
  }
}

}  // namespace

extern "C" int pcfa_fgsm_step_max_threads(void) { return FGSM_MAX_BLOCKS * FGSM_THREADS; }

extern "C" int pcfa_fgsm_step(float* x1, float* x2, const float* g1, const float* g2, const float* img1, const float* img2,
                              float* d1, float* d2, float epsilon, int joint, long long n, void* stream) {
  if (!x1 || !x2 || !g1 || !g2 || !img1 || !img2 || !d1 || !d2 || n < 0 || (joint != 0 && joint != 1))
    return PCFA_ERR_INVALID_ARG;
  if (n == 0) return PCFA_OK;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(x1) | reinterpret_cast<uintptr_t>(x2) | reinterpret_cast<uintptr_t>(g1) |
                         reinterpret_cast<uintptr_t>(g2) | reinterpret_cast<uintptr_t>(img1) |
                         reinterpret_cast<uintptr_t>(img2) | reinterpret_cast<uintptr_t>(d1) | reinterpret_cast<uintptr_t>(d2);
  const bool vec = (bits & 15) == 0 && n >= 4;
  long long blocks = ((vec ? (n + 3) / 4 : n) + FGSM_THREADS - 1) / FGSM_THREADS;
  if (blocks > FGSM_MAX_BLOCKS) blocks = FGSM_MAX_BLOCKS;
  if (vec)
    pcfa_launch(fgsm_step_kernel<true>, dim3((unsigned)blocks), dim3(FGSM_THREADS), 0, (hipStream_t)stream, x1, x2, g1, g2,
                img1, img2, d1, d2, epsilon, joint, n);
  else
    pcfa_launch(fgsm_step_kernel<false>, dim3((unsigned)blocks), dim3(FGSM_THREADS), 0, (hipStream_t)stream, x1, x2, g1, g2,
                img1, img2, d1, d2, epsilon, joint, n);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

// ---------------------------------------------------------------- projected-gradient step under the averaged-L2 budget
// attack_FGSM.pgd_l2_attack_step in three launches on one stream (include/pcfa_hip.h states the arithmetic):
//   1. pgd_l2_gsq_kernel    workgroup partials of G = sum g1^2 + sum g2^2
//   2. pgd_l2_step_kernel   every workgroup adds the G partials (the same order everywhere, so the same a), writes
//                           y = clamp(x - a g, 0, 1) and e = y - img into x and d, and its partial of E = sum e^2
//   3. pgd_l2_project_kernel  every workgroup adds the E partials; s == 1 returns at once, else x and d are rewritten
// No atomics, no memset, nothing read by the host.  An element belongs to the quad q = i / 4 and a quad to the thread
// q % (workgroups * 256) whether the accesses are 16-byte ones or scalar ones, so the grid, the partials and every sum
// depend on n alone.  Sums are double: a thread adds its elements' squares (exact in double) in index order, g1 before
// g2; a wave adds by shuffles; the four waves go through LDS and are added in wave order; the partials are added
// lane-strided, then the same way.  Every partial slot a launch reads was written by the launch before it.
namespace {

constexpr int PGD_THREADS = 256;
constexpr int PGD_MAX_BLOCKS = 1024;
constexpr int PGD_SCALARS = 4;   // workspace doubles 0..3: G, a, E, s; then PGD_MAX_BLOCKS partials of G and as many of E

// One fp32 rounding each, never fused: the compiler contracts a * b + c into an fma by default and the *_rn intrinsics
// are plain operators to it (fgsm_one can live with that: its products are exact).  The pragma takes the `contract` flag
// off these operations, and an operation without the flag is not fused after inlining either.
__device__ __forceinline__ float pgd_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float pgd_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float pgd_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

__device__ __forceinline__ double pgd_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// the workgroup's sum, in every thread
__device__ __forceinline__ double pgd_block_sum(double v, double* smem /*[4]*/) {
  const double w = pgd_wave_sum(v);
  if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = w;
  __syncthreads();
  return ((smem[0] + smem[1]) + smem[2]) + smem[3];
}

__device__ __forceinline__ double pgd_sum_partials(const double* __restrict__ partial, int count, double* smem) {
  double v = 0.;
  for (int i = threadIdx.x; i < count; i += PGD_THREADS) v += partial[i];
  return pgd_block_sum(v, smem);
}

// quad q of an array of n floats; elements past n read as 0 (they add nothing to a sum) and are never stored
template <bool VEC>
__device__ __forceinline__ float4 pgd_load(const float* p, long long q, long long n) {
  const long long i = q << 2;
  if (VEC && i + 3 < n) return reinterpret_cast<const float4*>(p)[q];
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < n) v.x = p[i];
  if (i + 1 < n) v.y = p[i + 1];
  if (i + 2 < n) v.z = p[i + 2];
  if (i + 3 < n) v.w = p[i + 3];
  return v;
}

template <bool VEC>
__device__ __forceinline__ void pgd_store(float* p, long long q, long long n, float4 v) {
  const long long i = q << 2;
  if (VEC && i + 3 < n) {
    reinterpret_cast<float4*>(p)[q] = v;
    return;
  }
  if (i < n) p[i] = v.x;
  if (i + 1 < n) p[i + 1] = v.y;
  if (i + 2 < n) p[i + 2] = v.z;
  if (i + 3 < n) p[i + 3] = v.w;
}

// joint: both images move along 0.5f * (g1 + g2), the fp32 sum rounded first as in fgsm_one
__device__ __forceinline__ void pgd_grad(float& g1, float& g2, int joint) {
  if (joint) g1 = g2 = pgd_mul(0.5f, pgd_add(g1, g2));
}

__device__ __forceinline__ double pgd_sq(double acc, float v1, float v2) {
  acc += (double)v1 * (double)v1;
  acc += (double)v2 * (double)v2;
  return acc;
}

template <bool VEC>
__global__ __launch_bounds__(PGD_THREADS) void pgd_l2_gsq_kernel(const float* __restrict__ g1, const float* __restrict__ g2,
                                                                 int joint, long long n, double* __restrict__ partial_g) {
  __shared__ double smem[4];
  const long long nq = (n + 3) >> 2, stride = (long long)gridDim.x * PGD_THREADS;
  double acc = 0.;
  for (long long q = (long long)blockIdx.x * PGD_THREADS + threadIdx.x; q < nq; q += stride) {
    float4 a = pgd_load<VEC>(g1, q, n), b = pgd_load<VEC>(g2, q, n);
    pgd_grad(a.x, b.x, joint);
    pgd_grad(a.y, b.y, joint);
    pgd_grad(a.z, b.z, joint);
    pgd_grad(a.w, b.w, joint);
    acc = pgd_sq(pgd_sq(pgd_sq(pgd_sq(acc, a.x, b.x), a.y, b.y), a.z, b.z), a.w, b.w);
  }
  const double sum = pgd_block_sum(acc, smem);
  if (threadIdx.x == 0) partial_g[blockIdx.x] = sum;
}

// y = clamp(x - a * g, 0, 1): the product is rounded, then the difference (no fma); e = y - img.  a == 0 moves nothing:
// the product is not formed (0 * Inf and 0 * NaN would be NaN)
__device__ __forceinline__ void pgd_move(float x, float g, float img, float a, float& y, float& e) {
  y = fgsm_clamp01(pgd_sub(x, a == 0.f ? 0.f : pgd_mul(a, g)));
  e = pgd_sub(y, img);
}

template <bool VEC>
__global__ __launch_bounds__(PGD_THREADS) void pgd_l2_step_kernel(float* x1, float* x2, const float* __restrict__ g1,
                                                                  const float* __restrict__ g2,
                                                                  const float* __restrict__ img1,
                                                                  const float* __restrict__ img2, float* __restrict__ d1,
                                                                  float* __restrict__ d2, double epsilon, int joint,
                                                                  long long n, double* __restrict__ ws) {
  __shared__ double smem_g[4], smem_e[4];
  const double G = pgd_sum_partials(ws + PGD_SCALARS, gridDim.x, smem_g);
  // a = 0 where the gradient has no length to scale by (G is 0, NaN or Inf) or the factor has no fp32 value
  float a = 0.f;
  if (G > 0. && G < __builtin_inf()) {
    a = (float)(epsilon * sqrt((double)(2 * n) / G));
    if (!(a < __builtin_inff())) a = 0.f;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ws[0] = G;
    ws[1] = (double)a;
  }
  const long long nq = (n + 3) >> 2, stride = (long long)gridDim.x * PGD_THREADS;
  double acc = 0.;
  for (long long q = (long long)blockIdx.x * PGD_THREADS + threadIdx.x; q < nq; q += stride) {
    const float4 a1 = pgd_load<VEC>(x1, q, n), a2 = pgd_load<VEC>(x2, q, n);
    float4 b1 = pgd_load<VEC>(g1, q, n), b2 = pgd_load<VEC>(g2, q, n);
    const float4 c1 = pgd_load<VEC>(img1, q, n), c2 = pgd_load<VEC>(img2, q, n);
    pgd_grad(b1.x, b2.x, joint);
    pgd_grad(b1.y, b2.y, joint);
    pgd_grad(b1.z, b2.z, joint);
    pgd_grad(b1.w, b2.w, joint);
    float4 y1, y2, e1, e2;
    pgd_move(a1.x, b1.x, c1.x, a, y1.x, e1.x);
    pgd_move(a2.x, b2.x, c2.x, a, y2.x, e2.x);
    pgd_move(a1.y, b1.y, c1.y, a, y1.y, e1.y);
    pgd_move(a2.y, b2.y, c2.y, a, y2.y, e2.y);
    pgd_move(a1.z, b1.z, c1.z, a, y1.z, e1.z);
    pgd_move(a2.z, b2.z, c2.z, a, y2.z, e2.z);
    pgd_move(a1.w, b1.w, c1.w, a, y1.w, e1.w);
    pgd_move(a2.w, b2.w, c2.w, a, y2.w, e2.w);
    pgd_store<VEC>(x1, q, n, y1);
    pgd_store<VEC>(x2, q, n, y2);
    pgd_store<VEC>(d1, q, n, e1);
    pgd_store<VEC>(d2, q, n, e2);
    acc = pgd_sq(pgd_sq(pgd_sq(pgd_sq(acc, e1.x, e2.x), e1.y, e2.y), e1.z, e2.z), e1.w, e2.w);
  }
  const double sum = pgd_block_sum(acc, smem_e);
  if (threadIdx.x == 0) ws[PGD_SCALARS + PGD_MAX_BLOCKS + blockIdx.x] = sum;
}

// x = clamp(img + s * e, 0, 1), product then sum (no fma); d = x - img from the updated x
__device__ __forceinline__ void pgd_shrink(float img, float e, float s, float& x, float& d) {
  x = fgsm_clamp01(pgd_add(img, pgd_mul(s, e)));
  d = pgd_sub(x, img);
}

template <bool VEC>
__global__ __launch_bounds__(PGD_THREADS) void pgd_l2_project_kernel(float* __restrict__ x1, float* __restrict__ x2,
                                                                     const float* __restrict__ img1,
                                                                     const float* __restrict__ img2, float* d1, float* d2,
                                                                     double bound, long long n, double* __restrict__ ws) {
  __shared__ double smem[4];
  const double E = pgd_sum_partials(ws + PGD_SCALARS + PGD_MAX_BLOCKS, gridDim.x, smem);
  float s = 1.f;
  if (E < __builtin_inf()) {   // (false for NaN too: a non-finite E leaves the step as it is)
    const double r = sqrt(E / (double)(2 * n));
    if (r > bound) s = (float)(bound / r);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ws[2] = E;
    ws[3] = (double)s;
  }
  if (s == 1.f) return;   // inside the budget (or a quotient that rounds to 1): x = y and d = e stay, bit for bit
  const long long nq = (n + 3) >> 2, stride = (long long)gridDim.x * PGD_THREADS;
  for (long long q = (long long)blockIdx.x * PGD_THREADS + threadIdx.x; q < nq; q += stride) {
    const float4 c1 = pgd_load<VEC>(img1, q, n), c2 = pgd_load<VEC>(img2, q, n);
    const float4 e1 = pgd_load<VEC>(d1, q, n), e2 = pgd_load<VEC>(d2, q, n);
    float4 y1, y2, f1, f2;
    pgd_shrink(c1.x, e1.x, s, y1.x, f1.x);
    pgd_shrink(c2.x, e2.x, s, y2.x, f2.x);
    pgd_shrink(c1.y, e1.y, s, y1.y, f1.y);
    pgd_shrink(c2.y, e2.y, s, y2.y, f2.y);
    pgd_shrink(c1.z, e1.z, s, y1.z, f1.z);
    pgd_shrink(c2.z, e2.z, s, y2.z, f2.z);
    pgd_shrink(c1.w, e1.w, s, y1.w, f1.w);
    pgd_shrink(c2.w, e2.w, s, y2.w, f2.w);
    pgd_store<VEC>(x1, q, n, y1);
    pgd_store<VEC>(x2, q, n, y2);
    pgd_store<VEC>(d1, q, n, f1);
    pgd_store<VEC>(d2, q, n, f2);
  }
}

template <bool VEC>
int pgd_l2_launch(float* x1, float* x2, const float* g1, const float* g2, const float* img1, const float* img2, float* d1,
                  float* d2, float epsilon, float delta_bound, int joint, long long n, double* ws, hipStream_t s) {
  long long blocks = ((n + 3) / 4 + PGD_THREADS - 1) / PGD_THREADS;
  if (blocks > PGD_MAX_BLOCKS) blocks = PGD_MAX_BLOCKS;
  const dim3 grid((unsigned)blocks), wg(PGD_THREADS);
  pcfa_launch(pgd_l2_gsq_kernel<VEC>, grid, wg, 0, s, g1, g2, joint, n, ws + PGD_SCALARS);
  PCFA_LAUNCH_CHECK();
  pcfa_launch(pgd_l2_step_kernel<VEC>, grid, wg, 0, s, x1, x2, g1, g2, img1, img2, d1, d2, (double)epsilon, joint, n, ws);
  PCFA_LAUNCH_CHECK();
  pcfa_launch(pgd_l2_project_kernel<VEC>, grid, wg, 0, s, x1, x2, img1, img2, d1, d2, (double)delta_bound, n, ws);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

}  // namespace

extern "C" size_t pcfa_pgd_l2_workspace_bytes(void) { return sizeof(double) * (PGD_SCALARS + 2 * PGD_MAX_BLOCKS); }

extern "C" int pcfa_pgd_l2_max_threads(void) { return PGD_MAX_BLOCKS * PGD_THREADS; }

extern "C" int pcfa_pgd_l2_step(float* x1, float* x2, const float* g1, const float* g2, const float* img1, const float* img2,
                                float* d1, float* d2, float epsilon, float delta_bound, int joint, long long n,
                                void* workspace, void* stream) {
  if (!x1 || !x2 || !g1 || !g2 || !img1 || !img2 || !d1 || !d2 || !workspace || n < 0 || (joint != 0 && joint != 1))
    return PCFA_ERR_INVALID_ARG;
  if (!(epsilon > 0.f && epsilon < __builtin_inff()) || !(delta_bound > 0.f && delta_bound < __builtin_inff()))
    return PCFA_ERR_INVALID_ARG;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(x1) | reinterpret_cast<uintptr_t>(x2) | reinterpret_cast<uintptr_t>(g1) |
                         reinterpret_cast<uintptr_t>(g2) | reinterpret_cast<uintptr_t>(img1) |
                         reinterpret_cast<uintptr_t>(img2) | reinterpret_cast<uintptr_t>(d1) | reinterpret_cast<uintptr_t>(d2);
  if ((bits & 3) || (reinterpret_cast<uintptr_t>(workspace) & 7)) return PCFA_ERR_INVALID_ARG;
  if (n == 0) return PCFA_OK;
  if ((bits & 15) == 0)   // ONE decision for all accesses of all three launches
    return pgd_l2_launch<true>(x1, x2, g1, g2, img1, img2, d1, d2, epsilon, delta_bound, joint, n, (double*)workspace,
                               (hipStream_t)stream);
  return pgd_l2_launch<false>(x1, x2, g1, g2, img1, img2, d1, d2, epsilon, delta_bound, joint, n, (double*)workspace,
                              (hipStream_t)stream);
}
