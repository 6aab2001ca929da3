// RAFT/GMA correlation computed on demand, forward and backward, for gfx950.
//
// Replaces CorrBlock (reference models/raft/corr.py:12-50) by the arithmetic of the reference's
// AlternateCorrBlock (models/raft/corr.py:63-91): the all-pairs pyramid pyr[B*Q][slab] is never formed.
// Average pooling is linear, so the level-l correlation of query q at position p is
//     C_l(q, p) = <f1(q), pool_l(f2)(p)> / sqrt(D),
// and a lookup computes only the (2r+2)^2 window dot products it blends.  Memory is O(Q*D).
//
// 1/sqrt(D) placement: the forward scales each window dot product by 1/sqrt(D) before the blend (the value the all-pairs
// pyramid stores); the backward scales each position's gradient dC by 1/sqrt(D) before both products.
//
// Workspace (one per build, pcfa_corr_ondemand_workspace_bytes; sections 256-B aligned):
//   f1t    [B][Q][D]   fp32   channels-last copy of fmap1
//   pyr    [l][B][H_l][W_l][D] fp32, then one all-zero row (the target of every out-of-map window position)
//   acc    same rows as pyr, int64: the fixed-point scatter of ONE lookup's backward (zeroed by prepare, and again by
//          every convert pass)
//   df2    same rows as pyr, fp32: the level gradients summed over the lookups of a backward pass
//   df1    [B][Q][D] fp32: dfmap1 summed over the lookups (channels-last)
//   f1max, gmax [OD_NBLK] fp32 block maxima; shift: the int fixed-point exponent of the current lookup's backward
//
// Work decomposition (wave64):
//   forward  : workgroup = 16 consecutive queries x one level, 4 waves; a wave owns one query at a time.  Lane = 4
//              channels: per window position one 1-KB coalesced row load (D = 256) and 4 FMAs into one of 64 per-lane
//              partials; a butterfly (63 shuffles per 64 positions) leaves position k's sum on lane k.  The dot products
//              go to LDS, lane t blends tap t, the 16 queries' taps leave through LDS as 64-B runs along q.
//              Every query costs the same whatever the coordinates: there is no box, so no large-box path.
//   backward : workgroup = 4 queries x all levels; wave = one query.  dC (10x10 from the 81 tap gradients) in LDS, then per
//              window position lane d (channels d, d+64, ..): dfmap1 += dC * f2_l(p) in registers (the query owns it: a
//              plain read-modify-write, no atomics), and df2_l(p) += dC * f1(q) as fixed-point int64 atomics, one 512-B
//              contiguous wave-instruction per 64 channels.  A convert pass then adds acc into df2 in fp32 and re-zeroes acc.
// Fixed point (fixed_point.hpp): the unit of a lookup's backward is 2^-shift with
//   shift = 61 - ceil(log2 Q) - (ilogb(M) + 1),  M = 2 * max|grad_out| * max|fmap1| / sqrt(D),
// since |dC| <= max|grad_out| / sqrt(D) (the bilinear weights a position receives sum to <= 1) and at most Q queries of one
// image add into one position: |sum| < 2^61.  Every addend keeps >= 61 - log2(Q) bits below the largest (>= 41 at 8K).
// Either maximum can flag the lookup; dfmap1 then carries the NaN through its fp32 sums.
//
// Tiled execution (pcfa_corr_ondemand_fwd_tiled / _bwd_tiled, Config.ondemand_lookup = "tiled"; corr_ondemand_tiled.hpp).
// Neighbouring queries look at neighbouring windows: the union of the windows of an 8x8 tile of queries at one level is a
// box of P = bw * bh positions, small whenever the flow is locally smooth.
//   classify : one launch per lookup, one wave per tile, on the device (no read-back: capturable).  Entry (tile, level) of
//              the table `tab` (workspace, after `shift`; 16 B each) holds the box, or bw = 0 for the per-query route:
//              a live coordinate that is not finite or meets the +-1e8 guard, or P > OD_MAXP (64-bit product).  Out-of-map
//              box positions count towards P.
//   forward  : workgroup = tile x level.  S[64 x P] = F1 F2box^T on v_mfma_f32_32x32x2_f32; out-of-map positions and dead
//              query rows of an edge tile read the zero row.  Only each query's own (2r+2)^2 window of S is kept (26 KB of
//              LDS whatever P), scaled by 1/sqrt(D); the blend is od_fwd_kernel's expression.  Dead rows are never stored.
//   backward : workgroup = tile, looping over the levels on the matrix route.  Per chunk of 64 box positions dC[64 x 64] is
//              built in LDS from the tap gradients (a query fills its own window, out-of-map positions and the rest are 0),
//              dfmap1 += dC F2box (the tile owns its dfmap1 rows: one plain store at the end, honouring accumulate), and
//              dF2box = dC^T F1 goes element by element through fix_quantize / fix_add into acc: P * D atomics per pair
//              instead of 64 (2r+2)^2 D, exact zeros skipped, never an out-of-map position.
//   The per-query kernels run after the tile kernels with `tab` as their predicate and serve the other pairs; in the
//   backward they add to the dfmap1 rows the tile kernel wrote.  The launch order is fixed, no float atomics: two calls,
//   two processes and two pairs in flight give the same bits.  All of it stays fp32 (Config.mfma has no effect here).
//   OD_MAXP = 512: with only the windows kept, LDS does not bound P (26 KB forward, 39 KB backward: several workgroups
//   per CU fit the 160 KB); what P bounds is the matrix work per pair, P / (2r+2)^2 times the products the windows need.
//   512 keeps that factor at 5 and every box of a locally smooth flow (|d flow| < 1 per texel: 18 x 18 .. 21 x 21).
//   od_shift_kernel's budget holds: a tile partial is an fp32 sum of n <= 64 terms, each |dC f1| <= M / 2, so its
//   magnitude is at most n (1 + 64 u) M / 2; a position receives partials whose term counts sum to at most Q, hence
//   |sum| <= Q (1 + 2^-18) (M / 2) 2^shift + 0.5 per partial < 2^61 with the factor 2 the unit leaves (M < 2^(ilogb M + 1)).
#include "common.hpp"
#include "fixed_point.hpp"

namespace {

constexpr int OD_NBLK = 256;            // block maxima per |x| reduction
constexpr int OD_QT = 16;               // queries per forward workgroup
constexpr int OD_KMAX = 8;              // channels per lane in the backward: D <= 512
constexpr int OD_TW = 8, OD_TH = 8;     // tiled execution: queries per tile (raster order inside the tile)
constexpr int OD_MAXP = 512;            // box positions up to which a (tile, level) pair takes the matrix route

struct OdLayout {
  int B, D, H, W, L, Q;
  int h[PCFA_MAX_LEVELS], w[PCFA_MAX_LEVELS];
  long long prow[PCFA_MAX_LEVELS];      // first row of level l (a row = D floats; [b][y][x] inside a level)
  long long rows;                       // B * sum_l h_l w_l; pyr row `rows` is the zero row
  size_t o_f1t, o_pyr, o_acc, o_df2, o_df1, o_f1max, o_gmax, o_shift, o_tab, bytes;
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

bool make_od_layout(OdLayout& Lo, int B, int D, int H, int W, int L) {
  if (B < 1 || D < 4 || D > 4 * 64 * 2 || (D & 3) || H < 1 || W < 1 || L < 1 || L > PCFA_MAX_LEVELS) return false;
  if ((long long)H * W > 0x7fffffffLL) return false;
  Lo.B = B; Lo.D = D; Lo.H = H; Lo.W = W; Lo.L = L; Lo.Q = H * W;
  long long rows = 0;
  int h = H, w = W;
  for (int l = 0; l < PCFA_MAX_LEVELS; ++l) {
    if (l < L) {
      if (h < 1 || w < 1) return false;
      Lo.h[l] = h; Lo.w[l] = w; Lo.prow[l] = rows;
      rows += (long long)B * h * w;
      h /= 2; w /= 2;
    } else {
      Lo.h[l] = 0; Lo.w[l] = 0; Lo.prow[l] = rows;
    }
  }
  Lo.rows = rows;
  const size_t qd = (size_t)B * Lo.Q * D, pd = (size_t)rows * D;
  size_t o = 0;
  Lo.o_f1t = o;   o = align256(o + qd * 4);
  Lo.o_pyr = o;   o = align256(o + (pd + D) * 4);
  Lo.o_acc = o;   o = align256(o + pd * 8);
  Lo.o_df2 = o;   o = align256(o + pd * 4);
  Lo.o_df1 = o;   o = align256(o + qd * 4);
  Lo.o_f1max = o; o = align256(o + OD_NBLK * 4);
  Lo.o_gmax = o;  o = align256(o + OD_NBLK * 4);
  Lo.o_shift = o; o = align256(o + 4);
  Lo.o_tab = o;   o = align256(o + (size_t)B * pcfa_cdiv(H, OD_TH) * pcfa_cdiv(W, OD_TW) * L * 16);   // OdTile entries
  Lo.bytes = o;
  return true;
}

template <typename T>
T* at(void* ws, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(ws) + off); }
template <typename T>
const T* at(const void* ws, size_t off) { return reinterpret_cast<const T*>(static_cast<const char*>(ws) + off); }

}  // namespace
#include "corr_ondemand_tiled.hpp"   // OdTile, the classification and the tile kernels (and corr_window.hpp)
namespace {

// ---- prepare -----------------------------------------------------------------------------------------------------------
// [B][D][Q] -> [B][Q][D] through a 32 x 33 LDS tile; block (32, 8), grid (cdiv(Q,32), cdiv(D,32), B)
__global__ __launch_bounds__(256) void od_to_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int D,
                                                         int Q) {
  __shared__ float t[32][33];
  const int q0 = blockIdx.x * 32, d0 = blockIdx.y * 32, b = blockIdx.z;
  const float* s = src + (size_t)b * D * Q;
  float* o = dst + (size_t)b * Q * D;
  for (int k = threadIdx.y; k < 32; k += 8) {
    const int d = d0 + k, q = q0 + threadIdx.x;
    t[k][threadIdx.x] = (d < D && q < Q) ? s[(size_t)d * Q + q] : 0.f;
  }
  __syncthreads();
  for (int k = threadIdx.y; k < 32; k += 8) {
    const int q = q0 + k, d = d0 + threadIdx.x;
    if (q < Q && d < D) o[(size_t)q * D + d] = t[threadIdx.x][k];
  }
}

// level l+1 = F.avg_pool2d(level l, 2, 2) (floor), channels-last; one thread per output float
__global__ __launch_bounds__(256) void od_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int hin,
                                                      int win, int hout, int wout, int D, long long n) {
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    const int d = (int)(i % D);
    const long long r = i / D;
    const int X = (int)(r % wout);
    const long long r2 = r / wout;
    const int Y = (int)(r2 % hout);
    const long long b = r2 / hout;
    const float* p = in + ((b * hin + 2 * Y) * win + 2 * X) * D + d;
    const size_t rs = (size_t)win * D;
    out[i] = (p[0] + p[D] + p[rs] + p[rs + D]) * 0.25f;
  }
}

__global__ __launch_bounds__(256) void od_absmax_kernel(const float* __restrict__ x, long long n, float* __restrict__ bmax) {
  __shared__ float red[4];
  fix_absmax_share(x, n, bmax, red, [](long long) {});
}

// the fixed-point exponent of one lookup's backward (header comment); one block of 256 threads
__global__ __launch_bounds__(256) void od_shift_kernel(const float* __restrict__ f1max, const float* __restrict__ gmax,
                                                       int log2q, float inv_sqrt_d, int* __restrict__ shift) {
  __shared__ float red[4];
  float a = fix_bmax_share(f1max, OD_NBLK), g = fix_bmax_share(gmax, OD_NBLK);
  a = fix_block_absmax(a, red);
  g = fix_block_absmax(g, red);
  if (threadIdx.x != 0) return;
  if (a == fix_inf() || g == fix_inf()) {
    *shift = FIX_NONFINITE;
    return;
  }
  const double M = 2.0 * (double)a * (double)g * (double)inv_sqrt_d;
  int s = 0;
  if (M > 0.0) s = 61 - log2q - (ilogb(M) + 1);
  *shift = s < -1000 ? -1000 : (s > 1000 ? 1000 : s);
}

// ---- forward -----------------------------------------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(256) void od_fwd_kernel(OdLayout Lo, const float* __restrict__ f1t,
                                                     const float* __restrict__ pyr, const float* __restrict__ coords,
                                                     float* __restrict__ out, float inv_sqrt_d,
                                                     const OdTile* __restrict__ tab) {
  constexpr int N1 = 2 * R + 1, WIN = 2 * R + 2, NPOS = WIN * WIN, NB = (NPOS + 63) / 64, NT = N1 * N1;
  static_assert(NT <= 128, "two taps per lane");
  __shared__ float s_dot[4][NB * 64];
  __shared__ float s_out[NT][OD_QT];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int l = blockIdx.y, b = blockIdx.z, q0 = blockIdx.x * OD_QT;
  const int D = Lo.D, Q = Lo.Q, hl = Lo.h[l], wl = Lo.w[l];
  const float* zrow = pyr + (size_t)Lo.rows * D;
  const float* lvl = pyr + ((size_t)Lo.prow[l] + (size_t)b * hl * wl) * D;
  // tab (the tiled execution): a query whose (tile, level) pair took the matrix route is skipped, here and in the store
  if (tab != nullptr) {
    const int q = min(q0 + (int)(threadIdx.x % OD_QT), Q - 1);
    if (!__syncthreads_or(od_tile_of(tab, Lo, b, q, l).bw == 0)) return;
  }

  for (int k = 0; k < OD_QT / 4; ++k) {
    const int qi = k * 4 + wv;                   // the four waves work on neighbouring queries at the same time
    const int q = min(q0 + qi, Q - 1);           // queries past the end compute a duplicate that is never stored
    const bool mine = tab == nullptr || od_tile_of(tab, Lo, b, q, l).bw == 0;   // wave-uniform
    const float cx = coords[((size_t)b * 2) * Q + q], cy = coords[((size_t)b * 2 + 1) * Q + q];
    const Origin o = make_origin(cx, cy, l, R);
    const float* f1 = f1t + ((size_t)b * Q + q) * D;
#pragma unroll
    for (int nb = 0; nb < (mine ? NB : 0); ++nb) {
      float acc[64];
#pragma unroll
      for (int i = 0; i < 64; ++i) acc[i] = 0.f;
      for (int c = lane * 4; c < D; c += 256) {
        const float4 a = *reinterpret_cast<const float4*>(f1 + c);
#pragma unroll
        for (int i = 0; i < 64; ++i) {
          const int p = nb * 64 + i;
          if (p < NPOS) {
            const int X = o.x0 + p % WIN, Y = o.y0 + p / WIN;
            const bool ok = X >= 0 && X < wl && Y >= 0 && Y < hl;
            const float* row = ok ? lvl + ((size_t)Y * wl + X) * D : zrow;
            const float4 v = *reinterpret_cast<const float4*>(row + c);
            acc[i] = fmaf(a.w, v.w, fmaf(a.z, v.z, fmaf(a.y, v.y, fmaf(a.x, v.x, acc[i]))));
          }
        }
      }
      // butterfly: after the step of mask m a lane keeps m partials (upper lanes the upper half); position k ends on lane k
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const bool up = (lane & m) != 0;
#pragma unroll
        for (int i = 0; i < m; ++i) {
          const float send = up ? acc[i] : acc[i + m];
          const float keep = up ? acc[i + m] : acc[i];
          acc[i] = keep + __shfl_xor(send, m);
        }
      }
      s_dot[wv][nb * 64 + lane] = acc[0] * inv_sqrt_d;
    }
    __syncthreads();
    const BlendWeights w = blend_weights(o.fx, o.fy);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int t = lane + 64 * h;
      if (t < NT) {
        const int a = t / N1, bb = t % N1;       // a: x offset, bb: y offset (channel a*(2r+1) + b)
        const float* c0 = &s_dot[wv][bb * WIN + a];
        const float* c1 = c0 + WIN;
        s_out[t][qi] = blend4(c0[0], c0[1], c1[0], c1[1], w);
      }
    }
    __syncthreads();
  }
  const size_t C = (size_t)Lo.L * NT;
  for (int i = threadIdx.x; i < NT * OD_QT; i += 256) {
    const int t = i / OD_QT, qi = i % OD_QT, q = q0 + qi;
    if (q < Q && (tab == nullptr || od_tile_of(tab, Lo, b, q, l).bw == 0))
      out[((size_t)b * C + (size_t)l * NT + t) * Q + q] = s_out[t][qi];
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(256) void od_bwd_kernel(OdLayout Lo, const float* __restrict__ f1t,
                                                     const float* __restrict__ pyr, const float* __restrict__ coords,
                                                     const float* __restrict__ grad, float* __restrict__ df1,
                                                     long long* __restrict__ acc, const int* __restrict__ shiftp,
                                                     int accumulate, float inv_sqrt_d, const OdTile* __restrict__ tab) {
  constexpr int N1 = 2 * R + 1, WIN = 2 * R + 2, NPOS = WIN * WIN, NT = N1 * N1;
  static_assert(NPOS <= 128, "two window positions per lane");
  __shared__ float s_g[4][128];
  __shared__ float s_dc[4][128];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = blockIdx.y, D = Lo.D, Q = Lo.Q;
  const int q = blockIdx.x * 4 + wv;
  const bool live = q < Q;
  const int qc = live ? q : Q - 1;
  const int shift = *shiftp;
  const bool scatter = live && shift != FIX_NONFINITE;
  const double scale = ldexp(1.0, shift == FIX_NONFINITE ? 0 : shift);
  const float* f1 = f1t + ((size_t)b * Q + qc) * D;
  float f1v[OD_KMAX], g1[OD_KMAX];
#pragma unroll
  for (int k = 0; k < OD_KMAX; ++k) {
    const int d = lane + 64 * k;
    f1v[k] = d < D ? f1[d] : 0.f;
    g1[k] = 0.f;
  }
  const float cx = coords[((size_t)b * 2) * Q + qc], cy = coords[((size_t)b * 2 + 1) * Q + qc];
  const size_t C = (size_t)Lo.L * NT;
  bool any = tab == nullptr;   // tab (the tiled execution): levels on the matrix route are skipped (wave-uniform)
  for (int l = 0; l < Lo.L; ++l) {
    const bool mine = tab == nullptr || od_tile_of(tab, Lo, b, qc, l).bw == 0;
    any |= mine;
    const Origin o = make_origin(cx, cy, l, R);
    const int hl = Lo.h[l], wl = Lo.w[l];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int t = lane + 64 * h;
      s_g[wv][t] = t < NT ? grad[((size_t)b * C + (size_t)l * NT + t) * Q + qc] : 0.f;
    }
    __syncthreads();
    const BlendWeights w = blend_weights(o.fx, o.fy);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int p = lane + 64 * h;
      if (p < NPOS) {
        const int i = p % WIN, j = p / WIN;     // x / y offset of the position in the window
        const float* G = s_g[wv];
        // tap (a, bb) blends positions (a, bb) w00, (a+1, bb) w01, (a, bb+1) w10, (a+1, bb+1) w11
        float dc = 0.f;
        if (i < N1 && j < N1) dc += w.w00 * G[i * N1 + j];
        if (i >= 1 && j < N1) dc += w.w01 * G[(i - 1) * N1 + j];
        if (i < N1 && j >= 1) dc += w.w10 * G[i * N1 + j - 1];
        if (i >= 1 && j >= 1) dc += w.w11 * G[(i - 1) * N1 + j - 1];
        const int X = o.x0 + i, Y = o.y0 + j;
        const bool ok = X >= 0 && X < wl && Y >= 0 && Y < hl;
        s_dc[wv][p] = ok ? dc * inv_sqrt_d : 0.f;
      }
    }
    __syncthreads();
    const float* lvl = pyr + ((size_t)Lo.prow[l] + (size_t)b * hl * wl) * D;
    long long* alvl = acc + ((size_t)Lo.prow[l] + (size_t)b * hl * wl) * D;
    float gl[OD_KMAX];   // this level's share: fp32 chains of <= (2r+2)^2 terms, not L (2r+2)^2
#pragma unroll
    for (int k = 0; k < OD_KMAX; ++k) gl[k] = 0.f;
    for (int p = 0; p < (mine ? NPOS : 0); ++p) {
      const int X = o.x0 + p % WIN, Y = o.y0 + p / WIN;
      const float dc = s_dc[wv][p];
      if (X < 0 || X >= wl || Y < 0 || Y >= hl || dc == 0.f) continue;   // wave-uniform
      const size_t ro = ((size_t)Y * wl + X) * D;
      const double dcs = (double)dc * scale;
#pragma unroll
      for (int k = 0; k < OD_KMAX; ++k) {
        const int d = lane + 64 * k;
        if (d < D) {
          gl[k] = fmaf(dc, lvl[ro + d], gl[k]);
          if (scatter) fix_add(alvl + ro + d, f1v[k], dcs);   // f1 * (dC * 2^shift): the position's scale
        }
      }
    }
#pragma unroll
    for (int k = 0; k < OD_KMAX; ++k) g1[k] += gl[k];
    __syncthreads();
  }
  if (!live || !any) return;
  float* g = df1 + ((size_t)b * Q + q) * D;
#pragma unroll
  for (int k = 0; k < OD_KMAX; ++k) {
    const int d = lane + 64 * k;
    if (d < D) g[d] = accumulate ? g[d] + g1[k] : g1[k];
  }
}

// df2 (+)= acc * 2^-shift in fp32, acc = 0; a flagged lookup writes NaN
__global__ __launch_bounds__(256) void od_convert_kernel(long long* __restrict__ acc, float* __restrict__ df2, long long n,
                                                         const int* __restrict__ shiftp, int accumulate) {
  const int shift = *shiftp;
  const bool bad = shift == FIX_NONFINITE;
  const double inv = ldexp(1.0, bad ? 0 : -shift);
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    const float v = bad ? fix_qnan() : fix_to_float(acc[i], inv);
    df2[i] = accumulate ? df2[i] + v : v;
    acc[i] = 0;
  }
}

// ---- finish ------------------------------------------------------------------------------------------------------------
// dst[b][d][q] = sum_l 4^-l src_l[b][y>>l][x>>l][d] (levels in order; a level-l position exists for its children only up
// to 2^l * W_l, 2^l * H_l); PYR = false: dst = src [B][Q][D] transposed.  Block (32, 8): 32 queries x 32 channels.
template <bool PYR>
__global__ __launch_bounds__(256) void od_finish_kernel(OdLayout Lo, const float* __restrict__ src, float* __restrict__ dst) {
  __shared__ float t[32][33];
  const int q0 = blockIdx.x * 32, d0 = blockIdx.y * 32, b = blockIdx.z;
  const int D = Lo.D, Q = Lo.Q, W = Lo.W;
  for (int k = threadIdx.y; k < 32; k += 8) {
    const int q = q0 + k, d = d0 + threadIdx.x;
    float v = 0.f;
    if (q < Q && d < D) {
      if constexpr (PYR) {
        const int y = q / W, x = q - y * W;
        float wgt = 1.f;
        for (int l = 0; l < Lo.L; ++l) {
          const int Y = y >> l, X = x >> l;
          if (Y < Lo.h[l] && X < Lo.w[l]) {
            const float s = src[((size_t)Lo.prow[l] + ((size_t)b * Lo.h[l] + Y) * Lo.w[l] + X) * D + d];
            v = l == 0 ? s : v + s * wgt;
          }
          wgt *= 0.25f;
        }
      } else {
        v = src[((size_t)b * Q + q) * D + d];
      }
    }
    t[k][threadIdx.x] = v;
  }
  __syncthreads();
  for (int k = threadIdx.y; k < 32; k += 8) {
    const int d = d0 + k, q = q0 + threadIdx.x;
    if (q < Q && d < D) dst[((size_t)b * D + d) * Q + q] = t[threadIdx.x][k];
  }
}

unsigned stride_grid(long long n) {
  const long long g = (n + 255) / 256;
  return (unsigned)(g < 8192 ? (g < 1 ? 1 : g) : 8192);
}

int ceil_log2(long long v) {
  int s = 0;
  while ((1LL << s) < v) ++s;
  return s;
}

float inv_sqrt(int D) { return (float)(1.0 / sqrt((double)D)); }

int od_tiles(const OdLayout& Lo) { return pcfa_cdiv(Lo.H, OD_TH) * pcfa_cdiv(Lo.W, OD_TW); }

// tiled: classification, then the tile kernel, then the per-query kernel over the pairs the classification left to it
template <int R>
int launch_fwd(const OdLayout& Lo, const void* ws, const float* coords, float* out, bool tiled, hipStream_t s) {
  const OdTile* tab = nullptr;
  if (tiled) {
    // the table is the one writable section behind a const workspace: a lookup owns it from its classification on
    OdTile* wtab = at<OdTile>(const_cast<void*>(ws), Lo.o_tab);
    tab = wtab;
    pcfa_launch(od_classify_kernel<R>, dim3(od_tiles(Lo), Lo.B), dim3(64), 0, s, Lo, coords, wtab);
    PCFA_LAUNCH_CHECK();
    pcfa_launch(od_fwd_tile_kernel<R>, dim3(od_tiles(Lo), Lo.L, Lo.B), dim3(256), 0, s, Lo, at<float>(ws, Lo.o_f1t),
                at<float>(ws, Lo.o_pyr), coords, tab, out, inv_sqrt(Lo.D));
    PCFA_LAUNCH_CHECK();
  }
  pcfa_launch(od_fwd_kernel<R>, dim3(pcfa_cdiv(Lo.Q, OD_QT), Lo.L, Lo.B), dim3(256), 0, s, Lo,
              at<float>(ws, Lo.o_f1t), at<float>(ws, Lo.o_pyr), coords, out, inv_sqrt(Lo.D), tab);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

// tiled: the tile kernel writes every dfmap1 row first (honouring accumulate), the per-query kernel then adds the levels
// the classification left to it: a fixed launch order, so a fixed order of dfmap1's sums
template <int R>
int launch_bwd(const OdLayout& Lo, void* ws, const float* coords, const float* grad, int accumulate, bool tiled,
               hipStream_t s) {
  const OdTile* tab = nullptr;
  if (tiled) {
    OdTile* wtab = at<OdTile>(ws, Lo.o_tab);
    tab = wtab;
    pcfa_launch(od_classify_kernel<R>, dim3(od_tiles(Lo), Lo.B), dim3(64), 0, s, Lo, coords, wtab);
    PCFA_LAUNCH_CHECK();
    pcfa_launch(od_bwd_tile_kernel<R>, dim3(od_tiles(Lo), Lo.B), dim3(256), 0, s, Lo, (const float*)at<float>(ws, Lo.o_f1t),
                (const float*)at<float>(ws, Lo.o_pyr), coords, grad, tab, at<float>(ws, Lo.o_df1),
                at<long long>(ws, Lo.o_acc), (const int*)at<int>(ws, Lo.o_shift), accumulate, inv_sqrt(Lo.D));
    PCFA_LAUNCH_CHECK();
    accumulate = 1;
  }
  pcfa_launch(od_bwd_kernel<R>, dim3(pcfa_cdiv(Lo.Q, 4), Lo.B), dim3(256), 0, s, Lo, (const float*)at<float>(ws, Lo.o_f1t),
              (const float*)at<float>(ws, Lo.o_pyr), coords, grad, at<float>(ws, Lo.o_df1), at<long long>(ws, Lo.o_acc),
              (const int*)at<int>(ws, Lo.o_shift), accumulate, inv_sqrt(Lo.D), tab);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

}  // namespace

extern "C" size_t pcfa_corr_ondemand_workspace_bytes(int B, int D, int H, int W, int num_levels) {
  OdLayout Lo;
  return make_od_layout(Lo, B, D, H, W, num_levels) ? Lo.bytes : 0;
}

extern "C" int pcfa_corr_ondemand_prepare(const float* fmap1, const float* fmap2, void* workspace, int B, int D, int H,
                                          int W, int num_levels, void* stream) {
  OdLayout Lo;
  if (!fmap1 || !fmap2 || !workspace) return PCFA_ERR_INVALID_ARG;
  if (!make_od_layout(Lo, B, D, H, W, num_levels)) return PCFA_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  float* pyr = at<float>(workspace, Lo.o_pyr);
  const dim3 tg(pcfa_cdiv(Lo.Q, 32), pcfa_cdiv(D, 32), B);
  pcfa_launch(od_to_rows_kernel, tg, dim3(32, 8), 0, s, fmap1, at<float>(workspace, Lo.o_f1t), D, Lo.Q);
  PCFA_LAUNCH_CHECK();
  pcfa_launch(od_to_rows_kernel, tg, dim3(32, 8), 0, s, fmap2, pyr, D, Lo.Q);
  PCFA_LAUNCH_CHECK();
  for (int l = 1; l < num_levels; ++l) {
    const long long n = (long long)B * Lo.h[l] * Lo.w[l] * D;
    pcfa_launch(od_pool_kernel, dim3(stride_grid(n)), dim3(256), 0, s, (const float*)(pyr + Lo.prow[l - 1] * D),
                pyr + Lo.prow[l] * D, Lo.h[l - 1], Lo.w[l - 1], Lo.h[l], Lo.w[l], D, n);
    PCFA_LAUNCH_CHECK();
  }
  pcfa_launch(zero_fill_kernel<1>, dim3(1), dim3(256), 0, s, ZeroSpans<1>{{pyr + Lo.rows * D}, {(long long)D}});
  PCFA_LAUNCH_CHECK();
  // the fixed-point accumulator starts at 0; each bwd's convert pass leaves it at 0 again
  const long long nacc = 2 * Lo.rows * D;
  pcfa_launch(zero_fill_kernel<1>, dim3(stride_grid(nacc)), dim3(256), 0, s,
              ZeroSpans<1>{{at<float>(workspace, Lo.o_acc)}, {nacc}});
  PCFA_LAUNCH_CHECK();
  pcfa_launch(od_absmax_kernel, dim3(OD_NBLK), dim3(256), 0, s, fmap1, (long long)B * D * Lo.Q,
              at<float>(workspace, Lo.o_f1max));
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

namespace {
int od_fwd(const void* workspace, const float* coords, float* out, int B, int D, int H, int W, int num_levels, int radius,
           bool tiled, void* stream) {
  OdLayout Lo;
  if (!workspace || !coords || !out) return PCFA_ERR_INVALID_ARG;
  if (!make_od_layout(Lo, B, D, H, W, num_levels)) return PCFA_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  switch (radius) {
    case 1: return launch_fwd<1>(Lo, workspace, coords, out, tiled, s);
    case 2: return launch_fwd<2>(Lo, workspace, coords, out, tiled, s);
    case 3: return launch_fwd<3>(Lo, workspace, coords, out, tiled, s);
    case 4: return launch_fwd<4>(Lo, workspace, coords, out, tiled, s);
    default: return PCFA_ERR_UNSUPPORTED;
  }
}

int od_bwd(void* workspace, const float* coords, const float* grad_out, int accumulate, int B, int D, int H, int W,
           int num_levels, int radius, bool tiled, void* stream) {
  OdLayout Lo;
  if (!workspace || !coords || !grad_out) return PCFA_ERR_INVALID_ARG;
  if (!make_od_layout(Lo, B, D, H, W, num_levels) || radius < 1 || radius > 4) return PCFA_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const long long nacc = Lo.rows * D;
  long long* acc = at<long long>(workspace, Lo.o_acc);
  const int n1 = 2 * radius + 1;
  pcfa_launch(od_absmax_kernel, dim3(OD_NBLK), dim3(256), 0, s, grad_out, (long long)B * num_levels * n1 * n1 * Lo.Q,
              at<float>(workspace, Lo.o_gmax));
  PCFA_LAUNCH_CHECK();
  pcfa_launch(od_shift_kernel, dim3(1), dim3(256), 0, s, (const float*)at<float>(workspace, Lo.o_f1max),
              (const float*)at<float>(workspace, Lo.o_gmax), ceil_log2(Lo.Q), inv_sqrt(D), at<int>(workspace, Lo.o_shift));
  PCFA_LAUNCH_CHECK();
  int st = PCFA_OK;
  switch (radius) {
    case 1: st = launch_bwd<1>(Lo, workspace, coords, grad_out, accumulate, tiled, s); break;
    case 2: st = launch_bwd<2>(Lo, workspace, coords, grad_out, accumulate, tiled, s); break;
    case 3: st = launch_bwd<3>(Lo, workspace, coords, grad_out, accumulate, tiled, s); break;
    case 4: st = launch_bwd<4>(Lo, workspace, coords, grad_out, accumulate, tiled, s); break;
  }
  if (st != PCFA_OK) return st;
  pcfa_launch(od_convert_kernel, dim3(stride_grid(nacc)), dim3(256), 0, s, acc, at<float>(workspace, Lo.o_df2), nacc,
              (const int*)at<int>(workspace, Lo.o_shift), accumulate);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}
}  // namespace

extern "C" int pcfa_corr_ondemand_fwd(const void* workspace, const float* coords, float* out, int B, int D, int H, int W,
                                      int num_levels, int radius, void* stream) {
  return od_fwd(workspace, coords, out, B, D, H, W, num_levels, radius, false, stream);
}

extern "C" int pcfa_corr_ondemand_fwd_tiled(const void* workspace, const float* coords, float* out, int B, int D, int H,
                                            int W, int num_levels, int radius, void* stream) {
  return od_fwd(workspace, coords, out, B, D, H, W, num_levels, radius, true, stream);
}

extern "C" int pcfa_corr_ondemand_bwd(void* workspace, const float* coords, const float* grad_out, int accumulate, int B,
                                      int D, int H, int W, int num_levels, int radius, void* stream) {
  return od_bwd(workspace, coords, grad_out, accumulate, B, D, H, W, num_levels, radius, false, stream);
}

extern "C" int pcfa_corr_ondemand_bwd_tiled(void* workspace, const float* coords, const float* grad_out, int accumulate,
                                            int B, int D, int H, int W, int num_levels, int radius, void* stream) {
  return od_bwd(workspace, coords, grad_out, accumulate, B, D, H, W, num_levels, radius, true, stream);
}

extern "C" int pcfa_corr_ondemand_tile_geometry(int* tile_w, int* tile_h, int* max_positions) {
  if (!tile_w || !tile_h || !max_positions) return PCFA_ERR_INVALID_ARG;
  *tile_w = OD_TW; *tile_h = OD_TH; *max_positions = OD_MAXP;
  return PCFA_OK;
}

extern "C" int pcfa_corr_ondemand_tile_routes(const void* workspace, int B, int D, int H, int W, int num_levels,
                                              int* counts, void* stream) {
  OdLayout Lo;
  if (!workspace || !counts) return PCFA_ERR_INVALID_ARG;
  if (!make_od_layout(Lo, B, D, H, W, num_levels)) return PCFA_ERR_UNSUPPORTED;
  pcfa_launch(od_routes_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, at<OdTile>(workspace, Lo.o_tab),
              (long long)B * od_tiles(Lo), num_levels, counts);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}

extern "C" int pcfa_corr_ondemand_finish(const void* workspace, float* dfmap1, float* dfmap2, int B, int D, int H, int W,
                                         int num_levels, void* stream) {
  OdLayout Lo;
  if (!workspace || !dfmap1 || !dfmap2) return PCFA_ERR_INVALID_ARG;
  if (!make_od_layout(Lo, B, D, H, W, num_levels)) return PCFA_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const dim3 tg(pcfa_cdiv(Lo.Q, 32), pcfa_cdiv(D, 32), B);
  pcfa_launch(od_finish_kernel<false>, tg, dim3(32, 8), 0, s, Lo, at<float>(workspace, Lo.o_df1), dfmap1);
  PCFA_LAUNCH_CHECK();
  pcfa_launch(od_finish_kernel<true>, tg, dim3(32, 8), 0, s, Lo, at<float>(workspace, Lo.o_df2), dfmap2);
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}
