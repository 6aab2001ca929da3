// SpyNet's 7x7 / stride 1 / pad 3 convolutions (reference models/SpyNet/SpyNet.py:56-84) and their data gradients on the fp32
// matrix cores of gfx950, for frozen weights.
//
// Formulation: direct implicit GEMM, out[co][pixel] = sum_k Wp[co][k] . X[k][pixel] with k = (input channel, ky, kx).  The
// OUTPUT CHANNELS are the A operand (rows), the PIXELS the B operand (columns): a lane's accumulators are channels of ONE
// pixel, so every store instruction writes MT consecutive pixels of one channel row.  Two MFMA shapes:
//   MT = 32: v_mfma_f32_32x32x2_f32 (k pair = two input channels of one tap) for 32 and 64 output channels;
//   MT = 16: v_mfma_f32_16x16x4_f32 (k quad = four input channels of one tap) for <= 16 output channels (layer 4 and 5
//            forward, the 8- and 16-channel data gradients), so a 16-row layer does not leave half of a 32-row tile idle.
// A workgroup (4 waves) owns TY output rows x 64 pixels x COT output channels.  The K loop runs over chunks of CK = 4 input
// channels: the chunk's weights (packed on the host in operand order, one contiguous range) and its zero-padded input patch
// [CK][TY + 6][70] are staged in LDS; the next chunk is requested into registers before the current one is multiplied and
// written to LDS after it, so the global latency hides under the MFMAs.  Patch rows of one channel are padded so that the
// KS lane groups of an operand read (different channels, same tap) fall on disjoint LDS banks.
//
// The data gradient is the same convolution of grad_out with the 180-degree rotated, channel-transposed weight
// (ops.spynet.conv7x7_dgrad_weight), with the ReLU backward applied where the gradient is loaded (mask = the layer's
// saved output: g where mask > 0, else 0).  Every output element is one k-ordered chain of MFMA fmas from zero in the same
// order on every call: no split-K, no atomics, no scratch -- the same bits on every call, lane and stream.
#include <type_traits>
#include "common.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int C7_CK = 4;    // input channels per chunk
constexpr int C7_TX = 64;   // output pixels per row segment
constexpr int C7_NT = 256;  // threads per workgroup

constexpr int pad_mod64(int a, int r) { return a + ((r - a % 64) + 64) % 64; }   // smallest >= a that is r mod 64

template <int MT_, int NBLK_, int TY_>
struct C7Cfg {
  static constexpr int MT = MT_, NBLK = NBLK_, TY = TY_;
  static constexpr int KS = 64 / MT;                    // k per MFMA step (input channels of one tap)
  static constexpr int COT = NBLK * MT;                 // output channels per workgroup
  static constexpr int STEPS = (C7_CK / KS) * 49;       // MFMA steps per chunk
  static constexpr int WFL = NBLK * STEPS * 64;         // packed weight floats per chunk
  static constexpr int R = TY + 6, CW = C7_TX + 6, RS = 72;
  static constexpr int CHS = pad_mod64(R * RS, MT);     // channel stride: lane groups on disjoint banks
  static constexpr int PATCH = C7_CK * CHS;
  static constexpr int NTILE = TY * (C7_TX / MT), TPW = NTILE / 4;   // pixel tiles per workgroup / per wave
  static constexpr int NW4 = (WFL / 4 + C7_NT - 1) / C7_NT;          // float4 weight pieces per thread
  static constexpr int NPE = C7_CK * R * CW, NP = (NPE + C7_NT - 1) / C7_NT;   // patch elements per thread
  static constexpr int ACC = MT == 32 ? 16 : 4;
  static_assert(NTILE % 4 == 0 && C7_CK % KS == 0, "tiling");
};
using Cfg64 = C7Cfg<32, 2, 2>;   // 64 output channels (layer 2 forward, layer 3 data gradient)
using Cfg32 = C7Cfg<32, 1, 4>;   // 32 (layers 1 and 3 forward, layers 2 and 4 data gradient)
using Cfg16 = C7Cfg<16, 1, 4>;   // <= 16 (layers 4 and 5 forward, layers 1 and 5 data gradient)

template <class C>
using AccT = typename std::conditional<C::MT == 32, f32x16, f32x4>::type;

template <class C>
__device__ __forceinline__ AccT<C> mfma(float a, float b, const AccT<C>& acc) {
  if constexpr (C::MT == 32) return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
}

// chunk ch -> registers: the packed weights (float4 pieces) and the masked, zero-padded input patch
template <class C>
__device__ __forceinline__ void c7_load(float4 (&rw)[C::NW4], float (&rp)[C::NP], const float* __restrict__ wct,
                                        const float* __restrict__ xb, const float* __restrict__ mb, int ch, int Cin,
                                        int H, int W, size_t plane, int y0, int x0) {
  const int tid = threadIdx.x;
  const float4* src = reinterpret_cast<const float4*>(wct + (size_t)ch * C::WFL);
#pragma unroll
  for (int i = 0; i < C::NW4; ++i)   // (a clamped index here put rw in scratch memory)
    rw[i] = (i + 1 < C::NW4 || tid + C7_NT * i < C::WFL / 4) ? src[tid + C7_NT * i] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int i = 0; i < C::NP; ++i) {
    const int e = min(tid + C7_NT * i, C::NPE - 1);
    const int c = e / (C::R * C::CW), rem = e - c * (C::R * C::CW), r = rem / C::CW, col = rem - r * C::CW;
    const int ci = ch * C7_CK + c, iy = y0 + r - 3, ix = x0 + col - 3;
    const bool ok = ci < Cin && iy >= 0 && iy < H && ix >= 0 && ix < W;
    const size_t off = (size_t)min(ci, Cin - 1) * plane + (size_t)min(max(iy, 0), H - 1) * W + min(max(ix, 0), W - 1);
    float v = xb[off];
    if (mb) v = mb[off] > 0.f ? v : 0.f;
    rp[i] = ok ? v : 0.f;
  }
}

template <class C>
__device__ __forceinline__ void c7_store(const float4 (&rw)[C::NW4], const float (&rp)[C::NP], float* wl, float* pl) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < C::NW4; ++i) {
    const int e = tid + C7_NT * i;
    if (i + 1 < C::NW4 || e < C::WFL / 4) reinterpret_cast<float4*>(wl)[e] = rw[i];
  }
#pragma unroll
  for (int i = 0; i < C::NP; ++i) {
    const int e = tid + C7_NT * i;
    if (i + 1 < C::NP || e < C::NPE) {
      const int c = e / (C::R * C::CW), rem = e - c * (C::R * C::CW), r = rem / C::CW, col = rem - r * C::CW;
      pl[c * C::CHS + r * C::RS + col] = rp[i];
    }
  }
}

// x: [B][Cin][H][W]; mask (or null): same shape, x is taken where mask > 0; wp: packed (conv7x7_pack); bias: [Cout] or
// null; addend: [B][Cout][H][W] or null; out: [B][Cout][H][W] = act(conv + bias) + addend   (ReLU before the addend is not
// a SpyNet shape: relu and addend are not combined by the host).
template <class C>
__global__ __launch_bounds__(C7_NT) void conv7x7_kernel(const float* __restrict__ x, const float* __restrict__ mask,
                                                        const float* __restrict__ wp, const float* __restrict__ bias,
                                                        const float* __restrict__ addend, float* __restrict__ out, int Cin,
                                                        int Cout, int H, int W, int nchunk, int tiles_x, int relu) {
  __shared__ __attribute__((aligned(16))) float wl[C::WFL];
  __shared__ __attribute__((aligned(16))) float pl[C::PATCH];
  const int tid = threadIdx.x, lane = tid & 63, m = lane % C::MT, h = lane / C::MT;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ty_blk = blockIdx.x / tiles_x;
  const int y0 = ty_blk * C::TY, x0 = (blockIdx.x - ty_blk * tiles_x) * C7_TX;
  const int ct = blockIdx.y, b = blockIdx.z;
  const size_t plane = (size_t)H * W;
  const float* xb = x + (size_t)b * Cin * plane;
  const float* mb = mask ? mask + (size_t)b * Cin * plane : nullptr;
  const float* wct = wp + (size_t)ct * nchunk * C::WFL;

  float4 rw[C::NW4];
  float rp[C::NP];
  AccT<C> acc[C::NBLK][C::TPW];
#pragma unroll
  for (int nb = 0; nb < C::NBLK; ++nb)
#pragma unroll
    for (int t = 0; t < C::TPW; ++t)
#pragma unroll
      for (int r = 0; r < C::ACC; ++r) acc[nb][t][r] = 0.f;

  // LDS operand offsets of this lane's pixel tiles (tile T = wave + 4 t: row T / (TX / MT), column group T % (TX / MT))
  int boff[C::TPW];
#pragma unroll
  for (int t = 0; t < C::TPW; ++t) {
    const int T = wv + 4 * t, tr = T / (C7_TX / C::MT), tc = T % (C7_TX / C::MT);
    boff[t] = h * C::CHS + tr * C::RS + tc * C::MT + m;
  }

  c7_load<C>(rw, rp, wct, xb, mb, 0, Cin, H, W, plane, y0, x0);
  c7_store<C>(rw, rp, wl, pl);
  __syncthreads();
  for (int ch = 0; ch < nchunk; ++ch) {
    c7_load<C>(rw, rp, wct, xb, mb, min(ch + 1, nchunk - 1), Cin, H, W, plane, y0, x0);   // next chunk in flight under this one's MFMAs (the last requests itself again)
#pragma unroll
    for (int cq = 0; cq < C7_CK / C::KS; ++cq)
#pragma unroll
      for (int ky = 0; ky < 7; ++ky)
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) {
          const int s = (cq * 7 + ky) * 7 + kx;
          float a[C::NBLK], bv[C::TPW];
#pragma unroll
          for (int nb = 0; nb < C::NBLK; ++nb) a[nb] = wl[(nb * C::STEPS + s) * 64 + lane];
#pragma unroll
          for (int t = 0; t < C::TPW; ++t) bv[t] = pl[boff[t] + cq * C::KS * C::CHS + ky * C::RS + kx];
#pragma unroll
          for (int nb = 0; nb < C::NBLK; ++nb)
#pragma unroll
            for (int t = 0; t < C::TPW; ++t) acc[nb][t] = mfma<C>(a[nb], bv[t], acc[nb][t]);
        }
    __syncthreads();
    if (ch + 1 < nchunk) {
      c7_store<C>(rw, rp, wl, pl);
      __syncthreads();
    }
  }

  // epilogue: register r of lane (m, h) is output channel (r & 3) + 8 (r >> 2) + 4 h of the tile, pixel m
#pragma unroll
  for (int t = 0; t < C::TPW; ++t) {
    const int T = wv + 4 * t, tr = T / (C7_TX / C::MT), tc = T % (C7_TX / C::MT);
    const int y = y0 + tr, xx = x0 + tc * C::MT + m;
    if (y >= H || xx >= W) continue;
    const size_t pix = (size_t)y * W + xx;
#pragma unroll
    for (int nb = 0; nb < C::NBLK; ++nb)
#pragma unroll
      for (int r = 0; r < C::ACC; ++r) {
        const int co = ct * C::COT + nb * C::MT + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (co >= Cout) continue;
        float v = acc[nb][t][r];
        if (bias) v += bias[co];
        if (relu) v = v < 0.f ? 0.f : v;   // (NaN passes, as torch's relu)
        const size_t o = ((size_t)b * Cout + co) * plane + pix;
        if (addend) v += addend[o];
        out[o] = v;
      }
  }
}

int pick(int Cout) { return Cout <= 16 ? 16 : Cout <= 32 ? 32 : 64; }

template <class C>
long long packed_floats(int Cin, int Cout) {
  return (long long)pcfa_cdiv(Cout, C::COT) * pcfa_cdiv(Cin, C7_CK) * C::WFL;
}

template <class C>
int run(const float* x, const float* mask, const float* wp, const float* bias, const float* addend, float* out, int B,
        int Cin, int Cout, int H, int W, int relu, hipStream_t s) {
  const int tiles_x = pcfa_cdiv(W, C7_TX), tiles_y = pcfa_cdiv(H, C::TY);
  dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)pcfa_cdiv(Cout, C::COT), (unsigned)B);
  pcfa_launch(conv7x7_kernel<C>, grid, dim3(C7_NT), 0, s, x, mask, wp, bias, addend, out, Cin, Cout, H, W,
              pcfa_cdiv(Cin, C7_CK), tiles_x, relu);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

}  // namespace

extern "C" int pcfa_conv7x7_tile(int Cout, int* mt, int* cot) {
  if (Cout < 1 || !mt || !cot) return PCFA_ERR_INVALID_ARG;
  const int p = pick(Cout);
  *mt = p == 16 ? Cfg16::MT : p == 32 ? Cfg32::MT : Cfg64::MT;
  *cot = p == 16 ? Cfg16::COT : p == 32 ? Cfg32::COT : Cfg64::COT;
  return PCFA_OK;
}

extern "C" long long pcfa_conv7x7_packed_floats(int Cin, int Cout) {
  if (Cin < 1 || Cout < 1) return 0;
  switch (pick(Cout)) {
    case 16: return packed_floats<Cfg16>(Cin, Cout);
    case 32: return packed_floats<Cfg32>(Cin, Cout);
    default: return packed_floats<Cfg64>(Cin, Cout);
  }
}

extern "C" int pcfa_conv7x7(const float* x, const float* mask, const float* packed, const float* bias, const float* addend,
                            float* out, int B, int Cin, int Cout, int H, int W, int relu, void* stream) {
  if (!x || !packed || !out || B < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1) return PCFA_ERR_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(packed) & 15) return PCFA_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  switch (pick(Cout)) {
    case 16: return run<Cfg16>(x, mask, packed, bias, addend, out, B, Cin, Cout, H, W, relu, s);
    case 32: return run<Cfg32>(x, mask, packed, bias, addend, out, B, Cin, Cout, H, W, relu, s);
    default: return run<Cfg64>(x, mask, packed, bias, addend, out, B, Cin, Cout, H, W, relu, s);
  }
}
