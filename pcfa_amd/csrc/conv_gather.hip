// The direct convolutions of FlowNet2 (strided and transposed, reference models/FlowNet/submodules.py:7-36,
// Config.flownet2_ops = "hip") and of SpyNet (7x7 / stride 1 / pad 3, models/SpyNet/SpyNet.py:56-84, Config.spynet_ops = "hip")
// and their data gradients on the fp32 matrix cores of gfx950, for frozen weights.
//
// One kernel, two modes, both a direct implicit GEMM out[co][pixel] = sum_k Wp[co][k] . X[k][pixel] over
// k = (input channel, ty, tx).  The OUTPUT CHANNELS are the A operand (MFMA rows), the PIXELS the B operand (columns): a
// lane's accumulators are channels of ONE pixel, so every store instruction writes MT consecutive pixels of one channel
// row.  MT = 32 (v_mfma_f32_32x32x2_f32, k pair = two input channels of one tap) for more than 16 output channels, MT = 16
// (v_mfma_f32_16x16x4_f32, k quad) below, so a 16-row layer does not leave half of a 32-row tile idle.
//   gather (npar = 1):  out[a][c] = sum W[ty][tx] x[S a + off + ty][S c + off + tx], S = 1 or 2, off = -pad.
//                       Stride-2 k x k convolutions (k = 3, 5, 7), the data gradient of ConvTranspose2d(4, 2, 1)
//                       (a stride-2 4x4 convolution of grad_out with the deconvolution weight as it is), and SpyNet's
//                       7x7 layers (S = 1, pcfa_conv7x7; their data gradient is the same convolution of grad_out with
//                       the 180-degree rotated, channel-transposed weight, ops.spynet.conv7x7_dgrad_weight).
//   parity (npar = 4):  S = 1, output parity (ry, rx) = blockIdx.z % 4 owns the outputs (2 a + ry, 2 c + rx) and reads
//                       x[a + off_ry + ty][c + off_rx + tx] with its own T x T sub-kernel.  A stride-2 transposed
//                       convolution is exactly this: the forward of ConvTranspose2d(4, 2, 1) (T = 2) and the data
//                       gradient of a stride-2 k x k convolution (T = ceil(k / 2), shorter parities padded with zero taps).
//                       The sub-kernels are cut on the host (ops.flownet2.parity_weights).
// A workgroup (4 waves) owns PIX = TY x TX output pixels (TX = 64 for wide maps, 16 for the coarse ones) x COT output
// channels; an MFMA column block is MT consecutive pixels of the tile in row-major order.  The K loop runs over chunks of
// CK = 4 input channels, weights and the zero-padded input patch of the chunk staged in LDS, the next chunk requested into
// registers before the current one is multiplied and written to LDS after it, so the global latency hides under the MFMAs.
// Patch rows of one channel are padded so that the KS lane groups of an operand read (different channels, same tap) fall
// on disjoint LDS banks.  With S = 2 the patch rows are stored de-interleaved (even columns, then odd columns), so the 32
// lanes of a B read fall on consecutive LDS words.
//
// Epilogue: + bias, ReLU (act == 1) or LeakyReLU(slope) (act == 2), + addend.  The data gradient applies the layer's
// activation backward where grad_out is loaded (mask = the layer's saved output: g where mask > 0, else g * mask_slope for
// the LeakyReLU, a select of 0 for SpyNet's ReLU, so that a non-finite g under the mask contributes exactly 0).  Every output
// element is one k-ordered chain of MFMAs from zero, the same on every call: no split-K, no atomics, no scratch.
#include <type_traits>
#include "common.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CG_CK = 4;    // input channels per chunk
constexpr int CG_NT = 256;  // threads per workgroup

constexpr int cg_pad_mod64(int a, int r) { return a + ((r - a % 64) + 64) % 64; }   // smallest >= a that is r mod 64

template <int MT_, int NBLK_, int PIX_, int TX_, int S_, int T_>
struct CgCfg {
  static constexpr int MT = MT_, NBLK = NBLK_, PIX = PIX_, TX = TX_, S = S_, T = T_;
  static constexpr int TY = PIX / TX;
  static constexpr int KS = 64 / MT;                     // k per MFMA step (input channels of one tap)
  static constexpr int COT = NBLK * MT;                  // output channels per workgroup
  static constexpr int STEPS = (CG_CK / KS) * T * T;     // MFMA steps per chunk
  static constexpr int WFL = NBLK * STEPS * 64;          // packed weight floats per chunk
  static constexpr int R = (TY - 1) * S + T, CW = (TX - 1) * S + T;   // input patch rows / columns
  static constexpr int HALF = S == 2 ? (CW + 1) / 2 : CW;              // de-interleaved half row (S = 2)
  // SpyNet's instance.  Its ReLU, addend and zero-select mask are compiled into this instance alone: as run-time branches
  // of every instance they cost the stride-2 kernels 2-12 VGPRs and two of them a wave of occupancy (FlowNet2 -1 %).
  static constexpr bool SPY = S == 1 && T == 7;
  static constexpr int RS = S == 2 ? 2 * HALF : SPY ? 72 : CW;         // LDS row stride (SpyNet: 72, as it was measured)
  static constexpr int CHS = cg_pad_mod64(R * RS, MT);   // channel stride: the KS lane groups on disjoint banks
  static constexpr int PATCH = CG_CK * CHS;
  static constexpr int NTILE = PIX / MT, TPW = NTILE / 4;             // pixel tiles per workgroup / per wave
  static constexpr int NW4 = (WFL / 4 + CG_NT - 1) / CG_NT;           // float4 weight pieces per thread
  static constexpr int NPE = CG_CK * R * CW, NP = (NPE + CG_NT - 1) / CG_NT;   // patch elements per thread
  static constexpr int ACC = MT == 32 ? 16 : 4;
  static_assert(NTILE % 4 == 0 && CG_CK % KS == 0 && PIX % TX == 0, "tiling");
  static_assert((WFL + PATCH) * 4 <= 160 * 1024, "LDS");
  static __device__ __forceinline__ int lcol(int col) { return S == 2 ? (col & 1) * HALF + (col >> 1) : col; }
};

template <class C>
using AccT = typename std::conditional<C::MT == 32, f32x16, f32x4>::type;

template <class C>
__device__ __forceinline__ AccT<C> mfma(float a, float b, const AccT<C>& acc) {
  if constexpr (C::MT == 32) return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
}

struct CgArgs {
  const float* x;      // [B][Cin][H][W]
  const float* mask;   // same shape or null: mask > 0 ? x : x * mslope (SpyNet's instance: mask > 0 ? x : 0)
  const float* wp;     // packed weights: [npar][Cout / cot][Cin / 4][cot / mt][4 / ks][T][T][ks][mt]
  const float* bias;   // [Cout] or null
  const float* addend; // [B][Cout][OH][OW] or null, added after the activation (SpyNet's instance)
  float* out;          // [B][Cout][OH][OW]
  int Cin, H, W, Cout, OH, OW;
  int npar, off0, off1;   // gather: npar 1, off0 = -pad; parity: npar 4, off0 / off1 = input offset of parity 0 / 1
  int nchunk, ncot, tiles_x;
  int act;                // after the bias: 1 ReLU (SpyNet's instance), 2 LeakyReLU(slope)
  float slope, mslope;
};

template <class C>
__device__ __forceinline__ void cg_load(float4 (&rw)[C::NW4], float (&rp)[C::NP], const float* __restrict__ wct,
                                        const float* __restrict__ xb, const float* __restrict__ mb, float mslope, int ch,
                                        int Cin, int H, int W, size_t plane, int iy0, int ix0) {
  const int tid = threadIdx.x;
  const float4* src = reinterpret_cast<const float4*>(wct + (size_t)ch * C::WFL);
#pragma unroll
  for (int i = 0; i < C::NW4; ++i)   // (a clamped index here put rw in scratch memory)
    rw[i] = (i + 1 < C::NW4 || tid + CG_NT * i < C::WFL / 4) ? src[tid + CG_NT * i] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int i = 0; i < C::NP; ++i) {
    const int e = min(tid + CG_NT * i, C::NPE - 1);
    const int c = e / (C::R * C::CW), rem = e - c * (C::R * C::CW), r = rem / C::CW, col = rem - r * C::CW;
    const int ci = ch * CG_CK + c, iy = iy0 + r, ix = ix0 + col;
    const bool ok = ci < Cin && iy >= 0 && iy < H && ix >= 0 && ix < W;
    const size_t off = (size_t)min(ci, Cin - 1) * plane + (size_t)min(max(iy, 0), H - 1) * W + min(max(ix, 0), W - 1);
    float v = xb[off];
    if (mb) v = mb[off] > 0.f ? v : C::SPY ? 0.f : v * mslope;   // (a select: a non-finite v under the mask gives exactly 0)
    rp[i] = ok ? v : 0.f;
  }
}

template <class C>
__device__ __forceinline__ void cg_store(const float4 (&rw)[C::NW4], const float (&rp)[C::NP], float* wl, float* pl) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < C::NW4; ++i) {
    const int e = tid + CG_NT * i;
    if (i + 1 < C::NW4 || e < C::WFL / 4) reinterpret_cast<float4*>(wl)[e] = rw[i];
  }
#pragma unroll
  for (int i = 0; i < C::NP; ++i) {
    const int e = tid + CG_NT * i;
    if (i + 1 < C::NP || e < C::NPE) {
      const int c = e / (C::R * C::CW), rem = e - c * (C::R * C::CW), r = rem / C::CW, col = rem - r * C::CW;
      pl[c * C::CHS + r * C::RS + C::lcol(col)] = rp[i];
    }
  }
}

template <class C>
__global__ __launch_bounds__(CG_NT) void conv_gather_kernel(CgArgs a) {
  __shared__ __attribute__((aligned(16))) float wl[C::WFL];
  __shared__ __attribute__((aligned(16))) float pl[C::PATCH];
  const int tid = threadIdx.x, lane = tid & 63, m = lane % C::MT, h = lane / C::MT;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int par = blockIdx.z % a.npar, b = blockIdx.z / a.npar;
  const int ry = par >> 1, rx = par & 1, os = a.npar == 4 ? 2 : 1;
  // logical output grid of this parity (all of the output in gather mode)
  const int OHl = a.npar == 4 ? (a.OH - ry + 1) / 2 : a.OH, OWl = a.npar == 4 ? (a.OW - rx + 1) / 2 : a.OW;
  const int offy = ry ? a.off1 : a.off0, offx = rx ? a.off1 : a.off0;
  const int ty_blk = blockIdx.x / a.tiles_x;
  const int y0 = ty_blk * C::TY, x0 = (blockIdx.x - ty_blk * a.tiles_x) * C::TX;
  const int iy0 = y0 * C::S + offy, ix0 = x0 * C::S + offx;
  const int ct = blockIdx.y;
  const size_t plane = (size_t)a.H * a.W;
  const float* xb = a.x + (size_t)b * a.Cin * plane;
  const float* mb = a.mask ? a.mask + (size_t)b * a.Cin * plane : nullptr;
  const float* wct = a.wp + ((size_t)par * a.ncot + ct) * a.nchunk * C::WFL;

  float4 rw[C::NW4];
  float rp[C::NP];
  AccT<C> acc[C::NBLK][C::TPW];
#pragma unroll
  for (int nb = 0; nb < C::NBLK; ++nb)
#pragma unroll
    for (int t = 0; t < C::TPW; ++t)
#pragma unroll
      for (int r = 0; r < C::ACC; ++r) acc[nb][t][r] = 0.f;

  // LDS operand offsets of this lane's pixel tiles (tile q = wave + 4 t covers tile pixels q * MT .. q * MT + MT - 1)
  int boff[C::TPW];
#pragma unroll
  for (int t = 0; t < C::TPW; ++t) {
    const int p = (wv + 4 * t) * C::MT + m, pr = p / C::TX, pc = p % C::TX;
    boff[t] = h * C::CHS + pr * C::S * C::RS + pc;
  }

  cg_load<C>(rw, rp, wct, xb, mb, a.mslope, 0, a.Cin, a.H, a.W, plane, iy0, ix0);
  cg_store<C>(rw, rp, wl, pl);
  __syncthreads();
  for (int ch = 0; ch < a.nchunk; ++ch) {
    cg_load<C>(rw, rp, wct, xb, mb, a.mslope, min(ch + 1, a.nchunk - 1), a.Cin, a.H, a.W, plane, iy0, ix0);
#pragma unroll
    for (int cq = 0; cq < CG_CK / C::KS; ++cq)
#pragma unroll
      for (int ky = 0; ky < C::T; ++ky)
#pragma unroll
        for (int kx = 0; kx < C::T; ++kx) {
          const int s = (cq * C::T + ky) * C::T + kx;
          const int toff = cq * C::KS * C::CHS + ky * C::RS + (C::S == 2 ? (kx & 1) * C::HALF + (kx >> 1) : kx);
          float av[C::NBLK], bv[C::TPW];
#pragma unroll
          for (int nb = 0; nb < C::NBLK; ++nb) av[nb] = wl[(nb * C::STEPS + s) * 64 + lane];
#pragma unroll
          for (int t = 0; t < C::TPW; ++t) bv[t] = pl[boff[t] + toff];
#pragma unroll
          for (int nb = 0; nb < C::NBLK; ++nb)
#pragma unroll
            for (int t = 0; t < C::TPW; ++t) acc[nb][t] = mfma<C>(av[nb], bv[t], acc[nb][t]);
        }
    __syncthreads();
    if (ch + 1 < a.nchunk) {
      cg_store<C>(rw, rp, wl, pl);
      __syncthreads();
    }
  }

  // epilogue: register r of lane (m, h) is output channel (r & 3) + 8 (r >> 2) + 4 h of the tile, pixel m
#pragma unroll
  for (int t = 0; t < C::TPW; ++t) {
    const int p = (wv + 4 * t) * C::MT + m, pr = p / C::TX, pc = p % C::TX;
    const int ya = y0 + pr, xa = x0 + pc;
    if (ya >= OHl || xa >= OWl) continue;
    const size_t pix = (size_t)(ya * os + ry) * a.OW + (xa * os + rx);
#pragma unroll
    for (int nb = 0; nb < C::NBLK; ++nb)
#pragma unroll
      for (int r = 0; r < C::ACC; ++r) {
        const int co = ct * C::COT + nb * C::MT + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (co >= a.Cout) continue;
        float v = acc[nb][t][r];
        if (a.bias) v += a.bias[co];
        if (C::SPY && a.act == 1) v = v < 0.f ? 0.f : v;   // (NaN passes, as torch's relu)
        if (a.act == 2) v = v > 0.f ? v : v * a.slope;
        const size_t o = ((size_t)b * a.Cout + co) * a.OH * a.OW + pix;
        if (C::SPY && a.addend) v += a.addend[o];
        a.out[o] = v;
      }
  }
}

// (mt, cot, pixels per workgroup) by output channels: 16 (<= 16 channels), 32, 64 (two 32-row blocks, half the pixels)
int pick(int Cout) { return Cout <= 16 ? 16 : Cout <= 32 ? 32 : 64; }

template <int S, int T, int TX>
int launch_tx(int p, CgArgs& a, int B, int OHl, int OWl, hipStream_t s) {
  auto go = [&](auto cfg) {
    using C = decltype(cfg);
    a.tiles_x = pcfa_cdiv(OWl, C::TX);
    a.ncot = pcfa_cdiv(a.Cout, C::COT);
    dim3 grid((unsigned)(a.tiles_x * pcfa_cdiv(OHl, C::TY)), (unsigned)a.ncot, (unsigned)(B * a.npar));
    pcfa_launch(conv_gather_kernel<C>, grid, dim3(CG_NT), 0, s, a);
    PCFA_LAUNCH_CHECK();
    return PCFA_OK;
  };
  switch (p) {
    case 16: return go(CgCfg<16, 1, 256, TX, S, T>{});
    case 32: return go(CgCfg<32, 1, 256, TX, S, T>{});
    default: return go(CgCfg<32, 2, 128, TX, S, T>{});
  }
}

template <int S, int T>
int launch_st(CgArgs& a, int B, int OHl, int OWl, hipStream_t s) {
  const int p = pick(a.Cout);
  if constexpr (S == 1 && T == 7) return launch_tx<S, T, 64>(p, a, B, OHl, OWl, s);   // SpyNet: 64-pixel segments on every map
  else return OWl >= 48 ? launch_tx<S, T, 64>(p, a, B, OHl, OWl, s) : launch_tx<S, T, 16>(p, a, B, OHl, OWl, s);
}

bool supported(int stride, int taps, int npar) {
  if (npar == 1) return (stride == 2 && (taps == 3 || taps == 4 || taps == 5 || taps == 7)) || (stride == 1 && taps == 3);
  return npar == 4 && stride == 1 && taps >= 2 && taps <= 4;
}

}  // namespace

extern "C" int pcfa_conv_gather_tile(int Cout, int* mt, int* cot) {
  if (Cout < 1 || !mt || !cot) return PCFA_ERR_INVALID_ARG;
  const int p = pick(Cout);
  *mt = p == 16 ? 16 : 32;
  *cot = p;
  return PCFA_OK;
}

extern "C" int pcfa_conv_gather_supported(int stride, int taps, int npar) { return supported(stride, taps, npar) ? 1 : 0; }

extern "C" long long pcfa_conv_gather_packed_floats(int Cin, int Cout, int taps, int npar) {
  if (Cin < 1 || Cout < 1 || taps < 1 || (npar != 1 && npar != 4)) return 0;
  const int cot = pick(Cout);
  return (long long)npar * pcfa_cdiv(Cout, cot) * cot * pcfa_cdiv(Cin, CG_CK) * CG_CK * taps * taps;
}

extern "C" int pcfa_conv_gather(const float* x, const float* mask, float mask_slope, const float* packed, const float* bias,
                                float* out, int B, int Cin, int H, int W, int Cout, int OH, int OW, int stride, int taps,
                                int npar, int off0, int off1, int act, float slope, void* stream) {
  if (!x || !packed || !out || B < 1 || Cin < 1 || H < 1 || W < 1 || Cout < 1 || OH < 1 || OW < 1)
    return PCFA_ERR_INVALID_ARG;
  if ((act != 0 && act != 2) || (reinterpret_cast<uintptr_t>(packed) & 15)) return PCFA_ERR_INVALID_ARG;
  if (!supported(stride, taps, npar)) return PCFA_ERR_UNSUPPORTED;
  if ((long long)B * npar > 65535) return PCFA_ERR_UNSUPPORTED;
  CgArgs a{x, mask, packed, bias, nullptr, out, Cin, H, W, Cout, OH, OW, npar, off0, off1, pcfa_cdiv(Cin, CG_CK), 0, 0, act,
           slope, mask_slope};
  const int OHl = npar == 4 ? (OH + 1) / 2 : OH, OWl = npar == 4 ? (OW + 1) / 2 : OW;   // parity 0: the largest
  hipStream_t s = (hipStream_t)stream;
  if (stride == 2) {
    switch (taps) {
      case 3: return launch_st<2, 3>(a, B, OHl, OWl, s);
      case 4: return launch_st<2, 4>(a, B, OHl, OWl, s);
      case 5: return launch_st<2, 5>(a, B, OHl, OWl, s);
      default: return launch_st<2, 7>(a, B, OHl, OWl, s);
    }
  }
  switch (taps) {
    case 2: return launch_st<1, 2>(a, B, OHl, OWl, s);
    case 3: return launch_st<1, 3>(a, B, OHl, OWl, s);
    default: return launch_st<1, 4>(a, B, OHl, OWl, s);
  }
}

// SpyNet's 7x7 / stride 1 / pad 3 layers: the S = 1, T = 7 gather instance with ReLU (act 1) and the addend.
extern "C" int pcfa_conv7x7_tile(int Cout, int* mt, int* cot) { return pcfa_conv_gather_tile(Cout, mt, cot); }

extern "C" long long pcfa_conv7x7_packed_floats(int Cin, int Cout) { return pcfa_conv_gather_packed_floats(Cin, Cout, 7, 1); }

extern "C" int pcfa_conv7x7(const float* x, const float* mask, const float* packed, const float* bias, const float* addend,
                            float* out, int B, int Cin, int Cout, int H, int W, int relu, void* stream) {
  if (!x || !packed || !out || B < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1) return PCFA_ERR_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(packed) & 15) return PCFA_ERR_INVALID_ARG;
  CgArgs a{x, mask, packed, bias, addend, out, Cin, H, W, Cout, H, W, 1, -3, 0, pcfa_cdiv(Cin, CG_CK), 0, 0, relu ? 1 : 0,
           0.f, 0.f};
  return launch_st<1, 7>(a, B, H, W, (hipStream_t)stream);
}
