// The dense GEMM core on the bf16 matrix cores with fp32 accuracy ("bf16x3", Config.mfma = "bf16x3") for gfx950.
//
// v_mfma_f32_32x32x2_f32 runs at 1/16 of the bf16 MFMA rate.  An fp32 number is exactly the sum of three bf16 numbers,
//   a = a0 + a1 + a2,   a0 = bf16(a), a1 = bf16(a - a0), a2 = bf16(a - a0 - a1)     (round to nearest; both
// subtractions exact), a product of two bf16 values is exact in fp32 and v_mfma_f32_32x32x16_bf16 accumulates in fp32.
// The six products a_i b_j with i + j <= 2 reproduce a b to 3.32 * 2^-26 |a b| (the dropped a1 b2, a2 b1, a2 b2), at
// 16 / 6 of the fp32 matrix roof.
//
// Same contract as pcfa_gemm_f32 / pcfa_corr_pyramid_fwd (corr_pyramid.hip) and the same block tile: 128x128, 4 waves
// (2x2), each wave 2x2 tiles of the 32x32 MFMA, so the epilogues of gemm_tile.hpp apply to the accumulators unchanged.
// Operands are read as fp32 and split ONCE per element on the way into LDS (three bf16 planes, 6 B per element; no
// pre-pass, no extra HBM traffic).  One stage = 16 k = one k-step of the MFMA: 12 ds_read_b128 and 24 MFMAs per wave.
//
// Summation order (fixed; no atomics): per 32x32 tile two accumulators, `hi` for a0 b0 and `lo` for the five small
// terms, which enter `lo` smallest first (i + j = 2: a0 b2, a1 b1, a2 b0; then i + j = 1: a0 b1, a1 b0).  `lo` is
// 2^-8 of `hi`, so its own roundings are far below fp32's; C = (hi + lo) * alpha.
//
// LDS image of one operand stage: [plane 3][k-half 2][row 128][8 bf16 = 16 B], k-half stride padded by 32 B.  Lane l
// of a wave reads (row l & 31, k-half l >> 5) = its MFMA fragment (A[row][k = 8 (l >> 5) + j]) as one ds_read_b128 from
// 512 contiguous bytes per half-wave: conflict-free.  Writers: a k-contiguous operand stores whole fragments (b128,
// thread = (row, k-half); 2-way on half of the lanes, hidden under the store's own transfer time), a k-major operand
// loads rows k and k + 1 and stores bf16 pairs (b32; 2-way, free for ds_write_b32).
#include "common.hpp"
#include "gemm_tile.hpp"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int XK = 16;                     // k per stage = k per v_mfma_f32_32x32x16_bf16
constexpr int HS = BM * 16 + 32;           // bytes between the two k-halves of a plane
constexpr int PLANE = 2 * HS;              // bytes per bf16 plane of an operand stage
constexpr int OPER = 3 * PLANE;            // bytes per operand stage
constexpr int STAGE_FLOATS = 2 * 2 * OPER / 4;   // A and B, double-buffered
static_assert(BM == BN, "one LDS image for both operands");

// a = p[0] + p[1] + p[2] exactly (|a| < 2^127; beyond, p[0] rounds to infinity and the rest is NaN)
__device__ __forceinline__ void split3(float a, __bf16 (&p)[3]) {
  p[0] = (__bf16)a;
  const float r1 = a - (float)p[0];
  p[1] = (__bf16)r1;
  const float r2 = r1 - (float)p[1];
  p[2] = (__bf16)r2;
}

// Stage one 128(dim) x 16(k) operand tile: global -> 8 floats per thread.
// KMAJ: stored [K][dim] (dim contiguous): thread = (k pair kp = tid & 7, 4 dims at 4 (tid >> 3)), r[e] = row k + e.
// else  stored [dim][K] (k contiguous):   thread = (row tid >> 1, k-half tid & 1),                r[e] = k + 4 e ..
// FAST (both dims % 4 == 0, 16-B aligned, K range % 4 == 0): unconditional float4 loads from clamped, always valid
// addresses -- no branch between a load and its use -- masked to zero before the split.
template <bool KMAJ>
__device__ __forceinline__ void x3_load_fast(const float* __restrict__ X, long long ld, int dim, int d0, int k0,
                                             int kend, float4 (&r)[2]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    if (KMAJ) {
      const int k = min(k0 + 2 * (tid & 7) + e, kend - 1), d = min(d0 + 4 * (tid >> 3), dim - 4);
      r[e] = *reinterpret_cast<const float4*>(X + (long long)k * ld + d);
    } else {
      const int d = min(d0 + (tid >> 1), dim - 1), k = min(k0 + 8 * (tid & 1) + 4 * e, kend - 4);
      r[e] = *reinterpret_cast<const float4*>(X + (long long)d * ld + k);
    }
  }
}

template <bool KMAJ>
__device__ __forceinline__ void x3_mask(int dim, int d0, int k0, int kend, float4 (&r)[2]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const bool ok = KMAJ ? (k0 + 2 * (tid & 7) + e < kend && d0 + 4 * (tid >> 3) < dim)
                         : (d0 + (tid >> 1) < dim && k0 + 8 * (tid & 1) + 4 * e < kend);
    if (!ok) r[e] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// The masked loader (misaligned or ragged operands): every element under its own predicate, exact zeros elsewhere.
template <bool KMAJ>
__device__ __forceinline__ void x3_load(const float* __restrict__ X, long long ld, int dim, int d0, int k0, int kend,
                                        float4 (&r)[2]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int k = KMAJ ? k0 + 2 * (tid & 7) + e : k0 + 8 * (tid & 1) + 4 * e + c;
      const int d = KMAJ ? d0 + 4 * (tid >> 3) + c : d0 + (tid >> 1);
      v[c] = 0.f;
      if (k < kend && d < dim) v[c] = KMAJ ? X[(long long)k * ld + d] : X[(long long)d * ld + k];
    }
    r[e] = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// Split the staged floats and write the three planes of the stage image at `s`.
template <bool KMAJ>
__device__ __forceinline__ void x3_store(char* __restrict__ s, const float4 (&r)[2]) {
  const int tid = threadIdx.x;
  const float v[2][4] = {{r[0].x, r[0].y, r[0].z, r[0].w}, {r[1].x, r[1].y, r[1].z, r[1].w}};
  if (KMAJ) {
    const int kp = tid & 7;
    char* dst = s + (kp >> 2) * HS + (4 * (tid >> 3)) * 16 + (kp & 3) * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      __bf16 lo[3], hi[3];
      split3(v[0][c], lo);   // row k
      split3(v[1][c], hi);   // row k + 1
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        bf16x2 w;
        w[0] = lo[p];
        w[1] = hi[p];
        *reinterpret_cast<bf16x2*>(dst + p * PLANE + c * 16) = w;
      }
    }
  } else {
    char* dst = s + (tid & 1) * HS + (tid >> 1) * 16;
    bf16x8 w[3];
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        __bf16 p3[3];
        split3(v[e][c], p3);
#pragma unroll
        for (int p = 0; p < 3; ++p) w[p][4 * e + c] = p3[p];
      }
#pragma unroll
    for (int p = 0; p < 3; ++p) *reinterpret_cast<bf16x8*>(dst + p * PLANE) = w[p];
  }
}

// C[m][n] = (sum_k A(m,k) B(k,n)) / div   over k in this block's split.
// grid = (ceil(N/128), ceil(M/128), batch*splits).  POOL: see PoolArgs (gemm_tile.hpp).
template <bool A_KM, bool B_KN, bool FAST, bool POOL>
__device__ __forceinline__ void gemm_bf16x3_body(
    const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ C, int M, int N, int K,
    long long lda, long long ldb, long long ldc, long long bsA, long long bsB, long long bsC, int splits, int kchunk,
    long long ssC, float div, const PoolArgs& pool) {
  constexpr int LDSF = POOL && BM * SC > STAGE_FLOATS ? BM * SC : STAGE_FLOATS;   // the C image reuses the stage buffers
  __shared__ __attribute__((aligned(16))) float smem[LDSF];
  char* const sbase = reinterpret_cast<char*>(smem);   // stage s: A at s * 2 * OPER, B at s * 2 * OPER + OPER

  const int batch = blockIdx.z / splits;
  const int split = blockIdx.z - batch * splits;
  A += batch * bsA;
  B += batch * bsB;
  C += batch * bsC + split * ssC;
  const int kbeg = split * kchunk;
  const int kend = min(K, kbeg + kchunk);
  int by = blockIdx.y, bx = blockIdx.x;
  gemm_tile_xcd_order(by, bx);
  const int m0 = by * BM;
  int n0 = bx * BN;
  bool pooled = false;
  if (POOL) {   // workgroup-uniform: a level-0 block (pooled epilogue) or a tail block (columns shifted to off_tail)
    if (bx < pool.nb0) {
      pooled = true;
      N = pool.S0;
    } else {
      n0 = pool.off_tail + (bx - pool.nb0) * BN;
    }
  }

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int l31 = lane & 31, lh = lane >> 5;

  f32x16 hi[2][2], lo[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        hi[i][j][r] = 0.f;
        lo[i][j][r] = 0.f;
      }

  float4 ra[2], rb[2];
  const int nk = (kend - kbeg + XK - 1) / XK;   // <= 0: a split past the end of K writes zeros
  if (nk > 0) {
    if (FAST) {
      x3_load_fast<A_KM>(A, lda, M, m0, kbeg, kend, ra);
      x3_load_fast<B_KN>(B, ldb, N, n0, kbeg, kend, rb);
      x3_mask<A_KM>(M, m0, kbeg, kend, ra);
      x3_mask<B_KN>(N, n0, kbeg, kend, rb);
    } else {
      x3_load<A_KM>(A, lda, M, m0, kbeg, kend, ra);
      x3_load<B_KN>(B, ldb, N, n0, kbeg, kend, rb);
    }
    x3_store<A_KM>(sbase, ra);
    x3_store<B_KN>(sbase + OPER, rb);
  }
  __syncthreads();
  int cur = 0;
  for (int kt = 0; kt < nk; ++kt) {
    const bool more = kt + 1 < nk;
    const int k0 = kbeg + (kt + 1) * XK;
    // the next tile is requested before the MFMA batch, and every load is issued before the first LDS write
    if (FAST) {  // unconditional: the stage past the end re-reads the last one (clamped) and is never read back
      x3_load_fast<A_KM>(A, lda, M, m0, min(k0, kend - 4), kend, ra);
      x3_load_fast<B_KN>(B, ldb, N, n0, min(k0, kend - 4), kend, rb);
      __builtin_amdgcn_sched_barrier(0);  // keep the loads ABOVE the MFMA block (hipcc otherwise sinks them to their use)
    } else if (more) {
      x3_load<A_KM>(A, lda, M, m0, k0, kend, ra);
      x3_load<B_KN>(B, ldb, N, n0, k0, kend, rb);
    }
    const char* sa = sbase + cur * 2 * OPER + lh * HS + (wr * 64 + l31) * 16;
    const char* sb = sbase + cur * 2 * OPER + OPER + lh * HS + (wc * 64 + l31) * 16;
    bf16x8 a[2][3], b[2][3];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        a[t][p] = *reinterpret_cast<const bf16x8*>(sa + p * PLANE + t * 32 * 16);
        b[t][p] = *reinterpret_cast<const bf16x8*>(sb + p * PLANE + t * 32 * 16);
      }
#define PCFA_X3_TERM(ACC, PA, PB)                                                                             \
  _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j)                  \
      ACC[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][PA], b[j][PB], ACC[i][j], 0, 0, 0)
    PCFA_X3_TERM(lo, 0, 2);   // i + j = 2, the smallest terms first
    PCFA_X3_TERM(lo, 1, 1);
    PCFA_X3_TERM(lo, 2, 0);
    PCFA_X3_TERM(lo, 0, 1);   // i + j = 1
    PCFA_X3_TERM(lo, 1, 0);
    PCFA_X3_TERM(hi, 0, 0);   // the leading term, apart from the small ones
#undef PCFA_X3_TERM
    if (FAST) {  // unconditional (also after the last stage, into the idle buffer): a store under `if (more)`
                 // lets hipcc sink the loads into that branch, i.e. below the MFMAs
      x3_mask<A_KM>(M, m0, k0, kend, ra);
      x3_mask<B_KN>(N, n0, k0, kend, rb);
      x3_store<A_KM>(sbase + (cur ^ 1) * 2 * OPER, ra);
      x3_store<B_KN>(sbase + (cur ^ 1) * 2 * OPER + OPER, rb);
    } else if (more) {
      x3_store<A_KM>(sbase + (cur ^ 1) * 2 * OPER, ra);
      x3_store<B_KN>(sbase + (cur ^ 1) * 2 * OPER + OPER, rb);
    }
    __syncthreads();
    cur ^= 1;
  }

#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) hi[i][j] += lo[i][j];
  gemm_tile_epilogue<POOL>(hi, smem, C, M, N, ldc, m0, n0, div, pooled, pool);
}

template <bool A_KM, bool B_KN, bool FAST>
__global__ __launch_bounds__(256, 2) void gemm_bf16x3_mfma_kernel(
    const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ C, int M, int N, int K,
    long long lda, long long ldb, long long ldc, long long bsA, long long bsB, long long bsC, int splits, int kchunk,
    long long ssC, float div) {
  gemm_bf16x3_body<A_KM, B_KN, FAST, false>(A, B, C, M, N, K, lda, ldb, ldc, bsA, bsB, bsC, splits, kchunk, ssC, div,
                                            PoolArgs{});
}

// The correlation pyramid's forward product with levels 1-2 pooled in the epilogue (see PoolArgs).
__global__ __launch_bounds__(256, 2) void corr_pyramid_pool_gemm_bf16x3_kernel(
    const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ C, int M, int N, int K,
    long long lda, long long ldb, long long ldc, long long bsA, long long bsB, long long bsC, float div,
    PoolArgs pool) {
  gemm_bf16x3_body<true, true, true, true>(A, B, C, M, N, K, lda, ldb, ldc, bsA, bsB, bsC, 1,
                                           ((K + XK - 1) / XK) * XK, 0LL, div, pool);
}

int x3_kchunk(int K, int splits) {
  const int per = (K + splits - 1) / splits;
  return ((per + XK - 1) / XK) * XK;
}

}  // namespace

extern "C" int pcfa_corr_pyramid_fwd_bf16x3(const float* fmap1, const float* f2ext, float* pyr, int B, int D, int H,
                                            int W, int num_levels, void* stream) {
  PyrLayout P;
  if (!fmap1 || !f2ext || !pyr || B < 1 || D < 1 || !pcfa_make_layout(P, H, W, num_levels))
    return PCFA_ERR_INVALID_ARG;
  const int Q = H * W, S = P.slab;
  const bool fast = Q % 4 == 0 && aligned16(fmap1) && aligned16(f2ext) && D % 4 == 0 && Q >= 4;   // slab % 16 == 0
  const float div = sqrtf((float)D);
  if (fast && P.L >= 3 && W % 16 == 0) {
    PoolArgs pa;
    if (!make_pool_args(P, pa)) return PCFA_ERR_UNSUPPORTED;
    dim3 gridp(pa.nb0 + pcfa_cdiv(S - pa.off_tail, BN), pcfa_cdiv(Q, BM), B);
    pcfa_launch(corr_pyramid_pool_gemm_bf16x3_kernel, gridp, dim3(256), 0, (hipStream_t)stream, fmap1, f2ext, pyr, Q,
                S, D, (long long)Q, (long long)S, (long long)S, (long long)D * Q, (long long)D * S, (long long)Q * S,
                div, pa);
    PCFA_LAUNCH_CHECK();
    return PCFA_OK;
  }
  dim3 grid(pcfa_cdiv(S, BN), pcfa_cdiv(Q, BM), B);
#define PCFA_GEMM_ARGS fmap1, f2ext, pyr, Q, S, D, (long long)Q, (long long)S, (long long)S, (long long)D * Q, \
                       (long long)D * S, (long long)Q * S, 1, ((D + XK - 1) / XK) * XK, 0LL, div
  if (fast)
    pcfa_launch(gemm_bf16x3_mfma_kernel<true, true, true>, grid, dim3(256), 0, (hipStream_t)stream, PCFA_GEMM_ARGS);
  else
    pcfa_launch(gemm_bf16x3_mfma_kernel<true, true, false>, grid, dim3(256), 0, (hipStream_t)stream, PCFA_GEMM_ARGS);
#undef PCFA_GEMM_ARGS
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" size_t pcfa_gemm_bf16x3_workspace_bytes(int M, int N, int batch, int splits) {
  if (M < 1 || N < 1 || batch < 1 || splits < 2) return 0;
  return sizeof(float) * (size_t)splits * batch * M * N;
}

extern "C" int pcfa_gemm_bf16x3(const float* A, const float* B, float* C, int M, int N, int K, long long lda,
                                long long ldb, long long ldc, int a_kmajor, int b_kmajor, int batch, long long bsA,
                                long long bsB, long long bsC, float alpha, int splits, void* workspace,
                                size_t workspace_bytes, void* stream) {
  if (!A || !B || !C || M < 1 || N < 1 || K < 1 || batch < 1 || splits < 1 || alpha == 0.f)
    return PCFA_ERR_INVALID_ARG;
  if (a_kmajor == 0 && b_kmajor != 0 && b_kmajor != 1) return PCFA_ERR_INVALID_ARG;
  if (a_kmajor == 1 && b_kmajor == 0) return PCFA_ERR_UNSUPPORTED;   // no call site; not instantiated
  hipStream_t s = (hipStream_t)stream;
  float* dst = C;
  long long bsD = bsC, ssD = 0, ldd = ldc;
  int kchunk = ((K + XK - 1) / XK) * XK;
  if (splits > 1) {
    if (!workspace || workspace_bytes < pcfa_gemm_bf16x3_workspace_bytes(M, N, batch, splits)) return PCFA_ERR_WORKSPACE;
    if (ldc != N || (batch > 1 && bsC != (long long)M * N)) return PCFA_ERR_UNSUPPORTED;   // dense C for the reduction
    dst = (float*)workspace;
    bsD = (long long)M * N;
    ssD = (long long)batch * M * N;
    ldd = N;
    kchunk = x3_kchunk(K, splits);
  }
  const bool vecA = aligned16(A) && lda % 4 == 0 && (a_kmajor ? M % 4 == 0 : K % 4 == 0) && bsA % 4 == 0;
  const bool vecB = aligned16(B) && ldb % 4 == 0 && (b_kmajor ? N % 4 == 0 : K % 4 == 0) && bsB % 4 == 0;
  const bool fast = vecA && vecB && K % 4 == 0 && M >= 4 && N >= 4 && K >= 4;
  dim3 grid(pcfa_cdiv(N, BN), pcfa_cdiv(M, BM), batch * splits);
  const float div = 1.0f / alpha;
#define PCFA_GEMM_ARGS A, B, dst, M, N, K, lda, ldb, ldd, bsA, bsB, bsD, splits, kchunk, ssD, div
#define PCFA_GEMM_GO(AK, BK_)                                                                                \
  do {                                                                                                       \
    if (fast) pcfa_launch(gemm_bf16x3_mfma_kernel<AK, BK_, true>, grid, dim3(256), 0, s, PCFA_GEMM_ARGS);    \
    else pcfa_launch(gemm_bf16x3_mfma_kernel<AK, BK_, false>, grid, dim3(256), 0, s, PCFA_GEMM_ARGS);        \
  } while (0)
  if (a_kmajor && b_kmajor) PCFA_GEMM_GO(true, true);
  else if (!a_kmajor && b_kmajor) PCFA_GEMM_GO(false, true);
  else PCFA_GEMM_GO(false, false);
#undef PCFA_GEMM_GO
#undef PCFA_GEMM_ARGS
  PCFA_LAUNCH_CHECK();
  if (splits > 1) {
    const long long n = (long long)batch * M * N;
    pcfa_launch(splitk_reduce_kernel, dim3(min(pcfa_cdiv(n, 256), 2048)), dim3(256), 0, s, (const float*)workspace, C,
                n, splits, n);
    PCFA_LAUNCH_CHECK();
  }
  return PCFA_OK;
}
