// GMA attention without the [N x N] matrix (Config.gma_attention = "streamed"), for gfx950.
//
// The materialised path (gma_ops.hip + pcfa_gemm_f32) holds attn = softmax(scale q k^T) as [N][N] fp32 from the forward
// to the end of the backward and adds two more matrices of that size in the backward.  Here every pass recomputes the
// 64 x 64 tile of logits it needs on the fp32 matrix cores (v_mfma_f32_32x32x2_f32, exact fp32 products) and consumes it
// at once; memory is O(N d).  The attention depends on the context features only, so the row statistic
//   lse_i = m_i + log sum_j exp(s_ij - m_i),     s_ij = scale * <q_i, k_j>,   m_i = max_j s_ij
// is computed once per forward (two sweeps: the exact maximum, then the sum) and every later pass forms
//   P_ij = exp(s_ij - lse_i)
// directly, with no online rescaling.  exp is the device expf of the HIP math library (documented within 1 ulp), the one
// pcfa_softmax_rows_fwd uses; the logit is rounded once after the scaling and once after the subtraction in every pass, so
// all passes see the same bits of s_ij (the products of a logit are summed in one fixed order everywhere).
//
// One kernel body serves all passes.  A workgroup (256 threads, 4 waves) OWNS a block of 64 rows and walks the other
// operand in blocks of 64 in ascending order:
//   lse : owns queries, streams keys     S = Q_own K_str^T                      -> m, sum per row
//   fwd : owns queries, streams keys     P = exp(S - lse[row]);  out += P V_str
//   dv  : owns keys,    streams queries  P^T = exp(K_own Q_str^T - lse[col]);   dv += P^T G_str
//   dq  : owns queries, streams keys     dS = P o (G_own V_str^T - delta[row]); dq += dS K_str      (times scale)
//   dk  : owns keys,    streams queries  dS^T = P^T o (V_own G_str^T - delta[col]); dk += dS^T Q_str (times scale)
// The S tile leaves the matrix cores in the accumulator layout, which is not the A-operand layout of the second product:
// it goes through LDS.  Rows and columns past N are loaded as zeros and their P / dS entries are forced to exactly 0.
// Every sum has one fixed order (ascending blocks, the k order of the tile product, a fixed shuffle tree): no atomics, no
// split whose finish depends on arrival order; two runs give equal bits.  All global offsets are 64-bit.
#include "common.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int D = 128;          // head dimension served
constexpr int BM = 64, BN = 64; // rows owned / rows streamed per step
constexpr int LD = D + 4;       // LDS row stride of a [64][128] tile (16-byte aligned rows, rows spread over the banks)
constexpr int LP = BN + 4;      // LDS row stride of the P tile
constexpr int NT = 256;
constexpr int TILE = BM * LD;
enum { MODE_LSE = 0, MODE_PV = 1, MODE_DS = 2 };
constexpr int LDS_FLOATS_PV = 3 * TILE + BM * LP + 4 * 64;
constexpr int LDS_FLOATS_DS = 4 * TILE + BM * LP + 4 * 64;

// 64 rows x 128 floats of g (row stride ld, column offset coff) starting at row0 into s; rows >= N become zeros
__device__ __forceinline__ void load_tile(float* s, const float* __restrict__ g, long long row0, int N, long long ld,
                                          int coff, int vec) {
#pragma unroll
  for (int i = 0; i < (BM * D / 4) / NT; ++i) {
    const int f = threadIdx.x + NT * i;
    const int r = f >> 5, c = (f & 31) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row0 + r < N) {
      const float* p = g + (row0 + r) * ld + coff + c;
      if (vec) {
        v = *reinterpret_cast<const float4*>(p);
      } else {
        v = make_float4(p[0], p[1], p[2], p[3]);
      }
    }
    *reinterpret_cast<float4*>(s + r * LD + c) = v;
  }
}

// acc += A[wr.., :] B[wc.., :]^T for two [64][128] LDS tiles, one 32 x 32 sub-tile per wave.  Lane l holds row l & 31 and
// the k half l >> 5; a 16-byte read feeds four matrix instructions (k = 8 t + 4 (l >> 5) + j): one fixed order of k.
__device__ __forceinline__ f32x16 tile_dot(const float* sa, const float* sb, int wr, int wc, int li, int lh, f32x16 acc) {
  const float* pa = sa + (wr + li) * LD + 4 * lh;
  const float* pb = sb + (wc + li) * LD + 4 * lh;
#pragma unroll 4
  for (int t = 0; t < D / 8; ++t) {
    const float4 a = *reinterpret_cast<const float4*>(pa + 8 * t);
    const float4 b = *reinterpret_cast<const float4*>(pb + 8 * t);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
  }
  return acc;
}

// X: the owned operand of the logits, Y: the streamed one.  W: the streamed operand of the second product (MODE_PV; in
// MODE_DS it is Y itself).  A2 / B2: owned / streamed operand of the [.. | ..] product, row stride n * D (MODE_DS).
// BYCOL: the row statistics belong to the streamed rows (dv, dk) instead of the owned ones.
template <int MODE, bool BYCOL>
__global__ __launch_bounds__(NT) void attn_stream_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                         const float* __restrict__ W, const float* __restrict__ A2,
                                                         const float* __restrict__ B2, const float* __restrict__ lse,
                                                         const float* __restrict__ delta, float* __restrict__ out,
                                                         int N, int n, float scale, int vec) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sX = smem;
  float* sY = sX + TILE;
  float* sP = sY + TILE;
  float* sStat = sP + BM * LP;   // [0,64) lse of owned rows, [64,128) of streamed rows, [128,192) / [192,256) delta
  float* sA = sStat + 4 * 64;
  float* sB = sA + TILE;         // MODE_DS only

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;   // this wave's 32 x 32 sub-tile of the 64 x 64 logits
  const int oc = (wave & 1) * 64;                          // and its two 32 x 32 sub-tiles of the 64 x 128 output
  const int li = lane & 31, lh = lane >> 5;
  const long long own0 = (long long)blockIdx.x * BM;
  const long long bh = blockIdx.y;
  const long long nd = (long long)n * D;
  X += bh * N * D;
  Y += bh * N * D;
  const int nblk = (N + BN - 1) / BN;

  load_tile(sX, X, own0, N, D, 0, vec);

  if (MODE == MODE_LSE) {
    // thread = (row, quarter of the 64 columns); the partial sum of a quarter runs over all key blocks in ascending
    // order and the four quarters are added as (p0 + p1) + (p2 + p3)
    const int row = tid >> 2, part = tid & 3;
    float m = -INFINITY, sum = 0.f;
    for (int sweep = 0; sweep < 2; ++sweep) {
      for (int jb = 0; jb < nblk; ++jb) {
        const long long col0 = (long long)jb * BN;
        load_tile(sY, Y, col0, N, D, 0, vec);
        __syncthreads();
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        acc = tile_dot(sX, sY, wr, wc, li, lh, acc);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int r = wr + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
          sP[r * LP + wc + li] = __fmul_rn(scale, acc[reg]);
        }
        __syncthreads();
        const float* ps = sP + row * LP + part * 16;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
          if (col0 + part * 16 + c < N) {
            const float s = ps[c];
            if (sweep == 0) m = fmaxf(m, s);
            else sum += expf(__fsub_rn(s, m));
          }
        }
      }
      if (sweep == 0) {
        m = fmaxf(m, __shfl_xor(m, 1));
        m = fmaxf(m, __shfl_xor(m, 2));
      }
    }
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    if (part == 0 && own0 + row < N) out[bh * N + own0 + row] = m + logf(sum);
    return;
  }

  W += bh * N * D;
  lse += bh * N;
  if (MODE == MODE_DS) {
    A2 += bh * N * nd;
    B2 += bh * N * nd;
    delta += bh * N;
  }
  if (!BYCOL && tid < BM) {
    const bool ok = own0 + tid < N;
    sStat[tid] = ok ? lse[own0 + tid] : 0.f;
    if (MODE == MODE_DS) sStat[128 + tid] = ok ? delta[own0 + tid] : 0.f;
  }

  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  f32x16 o0 = zero16, o1 = zero16;
  for (int jb = 0; jb < nblk; ++jb) {
    const long long col0 = (long long)jb * BN;
    __syncthreads();   // every read of the previous step's tiles is done
    load_tile(sY, Y, col0, N, D, 0, vec);
    if (BYCOL && tid < BN) {
      const bool ok = col0 + tid < N;
      sStat[64 + tid] = ok ? lse[col0 + tid] : 0.f;
      if (MODE == MODE_DS) sStat[192 + tid] = ok ? delta[col0 + tid] : 0.f;
    }
    f32x16 tacc = zero16;
    if (MODE == MODE_PV) {
      load_tile(sA, W, col0, N, D, 0, vec);
      __syncthreads();
    } else {
      for (int c = 0; c < n; ++c) {   // T = A2_own B2_str^T over the n chunks of 128, ascending
        if (c) __syncthreads();
        load_tile(sA, A2, own0, N, nd, c * D, vec);
        load_tile(sB, B2, col0, N, nd, c * D, vec);
        __syncthreads();
        tacc = tile_dot(sA, sB, wr, wc, li, lh, tacc);
      }
    }
    f32x16 acc = tile_dot(sX, sY, wr, wc, li, lh, zero16);
    {
      const int c = wc + li;
      const bool cok = col0 + c < N;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int r = wr + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
        const float st = BYCOL ? sStat[64 + c] : sStat[r];
        // a row or column past N contributes exactly 0, never exp(0 - lse)
        float p = (cok && own0 + r < N) ? expf(__fsub_rn(__fmul_rn(scale, acc[reg]), st)) : 0.f;
        if (MODE == MODE_DS) {
          const float dl = BYCOL ? sStat[192 + c] : sStat[128 + r];
          p = (cok && own0 + r < N) ? __fmul_rn(p, __fsub_rn(tacc[reg], dl)) : 0.f;
        }
        sP[r * LP + c] = p;
      }
    }
    __syncthreads();
    // out[64][128] += P[64][64] Wt[64][128]: two 32 x 32 sub-tiles per wave, k = streamed row, one fixed order
    const float* sW = (MODE == MODE_PV) ? sA : sY;
    const float* pp = sP + (wr + li) * LP + 4 * lh;
    const float* pw = sW + (4 * lh) * LD + oc + li;
#pragma unroll 2
    for (int t = 0; t < BN / 8; ++t) {
      const float4 a = *reinterpret_cast<const float4*>(pp + 8 * t);
      const float* w = pw + 8 * t * LD;
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, w[0], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, w[32], o1, 0, 0, 0);
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, w[LD], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, w[LD + 32], o1, 0, 0, 0);
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, w[2 * LD], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, w[2 * LD + 32], o1, 0, 0, 0);
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, w[3 * LD], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, w[3 * LD + 32], o1, 0, 0, 0);
    }
  }

  out += bh * N * D;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const long long r = own0 + wr + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
    if (r < N) {
      float* po = out + r * D + oc + li;
      po[0] = (MODE == MODE_DS) ? __fmul_rn(scale, o0[reg]) : o0[reg];
      po[32] = (MODE == MODE_DS) ? __fmul_rn(scale, o1[reg]) : o1[reg];
    }
  }
}

// delta[row] (+)= sum_c g[row][c] out[row][c]: one wave per row, lane-strided partial sums, a fixed shuffle tree
__global__ __launch_bounds__(NT) void attn_stream_delta_kernel(const float* __restrict__ g, const float* __restrict__ o,
                                                               float* __restrict__ delta, long long rows, int d,
                                                               int accumulate) {
  const long long row = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const float* pg = g + row * d;
  const float* po = o + row * d;
  float acc = 0.f;
  for (int c = lane; c < d; c += 64) acc = fmaf(pg[c], po[c], acc);
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s);
  if (lane == 0) delta[row] = accumulate ? delta[row] + acc : acc;
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int MODE, bool BYCOL>
int run(const float* X, const float* Y, const float* W, const float* A2, const float* B2, const float* lse,
        const float* delta, float* out, int BH, int N, int n, float scale, hipStream_t s) {
  constexpr int BYTES = (MODE == MODE_DS ? LDS_FLOATS_DS : LDS_FLOATS_PV) * (int)sizeof(float);
  static bool attr_set = false;   // > 64 KB of dynamic LDS needs the opt-in once per kernel
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)attn_stream_kernel<MODE, BYCOL>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, BYTES);
    if (e != hipSuccess) return (int)e;
    attr_set = true;
  }
  const int vec = al16(X) && al16(Y) && (!W || al16(W)) && (!A2 || al16(A2)) && (!B2 || al16(B2));
  dim3 grid((unsigned)((N + BM - 1) / BM), (unsigned)BH);
  pcfa_launch(attn_stream_kernel<MODE, BYCOL>, grid, dim3(NT), (size_t)BYTES, s, X, Y, W, A2, B2, lse, delta, out, N, n,
              scale, vec);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

int check_shape(int BH, int N, int d) {
  if (BH < 1 || N < 1 || d < 1 || BH > 65535) return PCFA_ERR_INVALID_ARG;
  if (d != D) return PCFA_ERR_UNSUPPORTED;
  return PCFA_OK;
}

}  // namespace

extern "C" int pcfa_attn_stream_lse(const float* q, const float* k, float* lse, int BH, int N, int d, float scale,
                                    void* stream) {
  if (!q || !k || !lse) return PCFA_ERR_INVALID_ARG;
  if (int e = check_shape(BH, N, d)) return e;
  return run<MODE_LSE, false>(q, k, nullptr, nullptr, nullptr, nullptr, nullptr, lse, BH, N, 1, scale,
                              (hipStream_t)stream);
}

extern "C" int pcfa_attn_stream_fwd(const float* q, const float* k, const float* v, const float* lse, float* out, int BH,
                                    int N, int d, float scale, void* stream) {
  if (!q || !k || !v || !lse || !out) return PCFA_ERR_INVALID_ARG;
  if (int e = check_shape(BH, N, d)) return e;
  return run<MODE_PV, false>(q, k, v, nullptr, nullptr, lse, nullptr, out, BH, N, 1, scale, (hipStream_t)stream);
}

extern "C" int pcfa_attn_stream_dv(const float* q, const float* k, const float* g, const float* lse, float* dv, int BH,
                                   int N, int d, float scale, void* stream) {
  if (!q || !k || !g || !lse || !dv) return PCFA_ERR_INVALID_ARG;
  if (int e = check_shape(BH, N, d)) return e;
  return run<MODE_PV, true>(k, q, g, nullptr, nullptr, lse, nullptr, dv, BH, N, 1, scale, (hipStream_t)stream);
}

extern "C" int pcfa_attn_stream_delta(const float* g, const float* out, float* delta, long long rows, int d,
                                      int accumulate, void* stream) {
  if (!g || !out || !delta || rows < 1 || d < 1 || rows > 0x7fffffffLL * (NT / 64)) return PCFA_ERR_INVALID_ARG;
  pcfa_launch(attn_stream_delta_kernel, dim3((unsigned)((rows + NT / 64 - 1) / (NT / 64))), dim3(NT), 0,
              (hipStream_t)stream, g, out, delta, rows, d, accumulate);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" int pcfa_attn_stream_dqk(const float* q, const float* k, const float* lse, const float* G, const float* V,
                                    const float* delta, float* dq, float* dk, int BH, int N, int d, int n, float scale,
                                    void* stream) {
  if (!q || !k || !lse || !G || !V || !delta || (!dq && !dk) || n < 1) return PCFA_ERR_INVALID_ARG;
  if (int e = check_shape(BH, N, d)) return e;
  if (dq)
    if (int e = run<MODE_DS, false>(q, k, k, G, V, lse, delta, dq, BH, N, n, scale, (hipStream_t)stream)) return e;
  if (dk)
    if (int e = run<MODE_DS, true>(k, q, q, V, G, lse, delta, dk, BH, N, n, scale, (hipStream_t)stream)) return e;
  return PCFA_OK;
}
