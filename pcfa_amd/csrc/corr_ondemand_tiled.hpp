// The tiled execution of the on-demand correlation lookup (Config.ondemand_lookup = "tiled"); included by
// corr_ondemand.hip after OdLayout, whose header comment states the decomposition and the budgets.
#pragma once
#include "corr_window.hpp"   // Origin / make_origin, the blend
#include "gemm_tile.hpp"     // f32x16 and the C/D register map of the 32x32 MFMA

namespace {

constexpr int OD_TQ = OD_TW * OD_TH;

// One entry per (image, tile, level): the box origin (level texels) and size; bw == 0: the per-query route.
struct OdTile {
  int bx0, by0, bw, bh;
};

__device__ __forceinline__ int od_tiles_x(int W) { return (W + OD_TW - 1) / OD_TW; }
__device__ __forceinline__ int od_tiles_y(int H) { return (H + OD_TH - 1) / OD_TH; }

// the entry of query (b, y, x) at level l
__device__ __forceinline__ const OdTile& od_tile_of(const OdTile* __restrict__ tab, const OdLayout& Lo, int b, int q, int l) {
  const int y = q / Lo.W, x = q - y * Lo.W;
  const int t = (y / OD_TH) * od_tiles_x(Lo.W) + x / OD_TW;
  return tab[((size_t)b * od_tiles_x(Lo.W) * od_tiles_y(Lo.H) + t) * Lo.L + l];
}

// C/D register r of lane half lh -> row of the 32x32 block (gemm_tile.hpp)
__device__ __forceinline__ int od_acc_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// ---- classification: one wave per tile, lane = query ---------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(64) void od_classify_kernel(OdLayout Lo, const float* __restrict__ coords,
                                                         OdTile* __restrict__ tab) {
  constexpr int WIN = 2 * R + 2;
  const int lane = threadIdx.x, b = blockIdx.y, t = blockIdx.x;
  const int ntx = od_tiles_x(Lo.W);
  const int y = (t / ntx) * OD_TH + lane / OD_TW, x = (t % ntx) * OD_TW + lane % OD_TW;
  const bool live = y < Lo.H && x < Lo.W;
  const int q = live ? y * Lo.W + x : 0;
  const float cx = coords[((size_t)b * 2) * Lo.Q + q], cy = coords[((size_t)b * 2 + 1) * Lo.Q + q];
  for (int l = 0; l < Lo.L; ++l) {
    const Origin o = make_origin(cx, cy, l, R);
    const float inv = 1.0f / (float)(1 << l);
    const float flx = floorf(cx * inv), fly = floorf(cy * inv);
    // finite and inside the guard (NaN fails both comparisons)
    int ok = !live || (fabsf(flx) < 1.0e8f && fabsf(fly) < 1.0e8f);
    int xmin = live ? o.x0 : 0x7fffffff, xmax = live ? o.x0 : (int)0x80000000;
    int ymin = live ? o.y0 : 0x7fffffff, ymax = live ? o.y0 : (int)0x80000000;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      xmin = min(xmin, __shfl_xor(xmin, m));
      xmax = max(xmax, __shfl_xor(xmax, m));
      ymin = min(ymin, __shfl_xor(ymin, m));
      ymax = max(ymax, __shfl_xor(ymax, m));
      ok &= __shfl_xor(ok, m);
    }
    if (lane == 0) {
      OdTile e{0, 0, 0, 0};
      if (ok) {
        const long long bw = (long long)xmax - xmin + WIN, bh = (long long)ymax - ymin + WIN;
        if (bw * bh <= OD_MAXP) e = OdTile{xmin, ymin, (int)bw, (int)bh};
      }
      tab[((size_t)b * gridDim.x + t) * Lo.L + l] = e;
    }
  }
}

// counts[l][0] = pairs of level l on the matrix route, counts[l][1] = on the per-query route; one block
__global__ __launch_bounds__(256) void od_routes_kernel(const OdTile* __restrict__ tab, long long tiles, int L,
                                                        int* __restrict__ counts) {
  __shared__ int c[PCFA_MAX_LEVELS][2];
  if (threadIdx.x < PCFA_MAX_LEVELS * 2) (&c[0][0])[threadIdx.x] = 0;
  __syncthreads();
  for (long long i = threadIdx.x; i < tiles * L; i += 256) atomicAdd(&c[i % L][tab[i].bw == 0], 1);
  __syncthreads();
  if ((int)threadIdx.x < L * 2) counts[threadIdx.x] = (&c[0][0])[threadIdx.x];
}

// ---- tile geometry shared by forward and backward --------------------------------------------------------------------------
struct OdTileQuery {
  int qx0, qy0;          // window origin of the query (level texels); dead queries: far outside every box
  float fx, fy;
};

// a float4 of a D-float row at channel c, zero past the row's end (address clamped, load unconditional)
__device__ __forceinline__ float4 od_load4(const float* __restrict__ row, int c, int D) {
  float4 v = *reinterpret_cast<const float4*>(row + min(c, D - 4));
  if (c >= D) v = make_float4(0.f, 0.f, 0.f, 0.f);
  return v;
}

// ---- forward: workgroup = tile x level ----------------------------------------------------------------------------------
// S[64 x P] = F1 F2box^T on v_mfma_f32_32x32x2_f32; wave w owns the column blocks (32 box positions) w, w + 4, ..  Both
// operands come straight from their channels-last rows, 16 B per lane: lane (r, h) holds channels 8 g + 4 h + e of row r
// in k-step e of channel group g, the same channel permutation on both sides.  Of S only each query's own window is kept
// (64 x (2r+2)^2 floats of LDS, whatever P).
template <int R>
__global__ __launch_bounds__(256) void od_fwd_tile_kernel(OdLayout Lo, const float* __restrict__ f1t,
                                                          const float* __restrict__ pyr, const float* __restrict__ coords,
                                                          const OdTile* __restrict__ tab, float* __restrict__ out,
                                                          float inv_sqrt_d) {
  constexpr int N1 = 2 * R + 1, WIN = 2 * R + 2, NPOS = WIN * WIN, NT = N1 * N1;
  __shared__ float s_win[OD_TQ][NPOS + 1];
  __shared__ OdTileQuery s_q[OD_TQ];
  const int t = blockIdx.x, l = blockIdx.y, b = blockIdx.z;
  const OdTile e = tab[((size_t)b * gridDim.x + t) * Lo.L + l];
  if (e.bw == 0) return;                         // per-query route: od_fwd_kernel serves the pair
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, lh = lane >> 5;
  const int D = Lo.D, Q = Lo.Q, hl = Lo.h[l], wl = Lo.w[l];
  const int ntx = od_tiles_x(Lo.W), ty0 = (t / ntx) * OD_TH, tx0 = (t % ntx) * OD_TW;
  const float* zrow = pyr + (size_t)Lo.rows * D;
  const float* lvl = pyr + ((size_t)Lo.prow[l] + (size_t)b * hl * wl) * D;
  const int P = e.bw * e.bh;

  if (threadIdx.x < OD_TQ) {
    const int y = ty0 + threadIdx.x / OD_TW, x = tx0 + threadIdx.x % OD_TW;
    OdTileQuery tq{-(1 << 30), -(1 << 30), 0.f, 0.f};
    if (y < Lo.H && x < Lo.W) {
      const int q = y * Lo.W + x;
      const Origin o = make_origin(coords[((size_t)b * 2) * Q + q], coords[((size_t)b * 2 + 1) * Q + q], l, R);
      tq = OdTileQuery{o.x0, o.y0, o.fx, o.fy};
    }
    s_q[threadIdx.x] = tq;
  }
  __syncthreads();

  // rows of the A operand: query r and r + 32 of the tile (dead rows read the zero row)
  const float* arow[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int qi = i * 32 + r, y = ty0 + qi / OD_TW, x = tx0 + qi % OD_TW;
    arow[i] = (y < Lo.H && x < Lo.W) ? f1t + ((size_t)b * Q + (size_t)y * Lo.W + x) * D : zrow;
  }
  const int ncb = (P + 31) / 32;
  for (int cb = wv; cb < ncb; cb += 4) {
    const int p = cb * 32 + r;
    const int py = p / e.bw, px = p - py * e.bw;
    const int X = e.bx0 + px, Y = e.by0 + py;
    const bool inmap = p < P && X >= 0 && X < wl && Y >= 0 && Y < hl;
    const float* brow = inmap ? lvl + ((size_t)Y * wl + X) * D : zrow;
    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[i][k] = 0.f;
    float4 a0 = od_load4(arow[0], 4 * lh, D), a1 = od_load4(arow[1], 4 * lh, D), bv = od_load4(brow, 4 * lh, D);
    for (int c = 0; c < D; c += 8) {
      // the next group's loads are requested before this group's MFMA batch
      const int cn = c + 8 + 4 * lh;
      const float4 na0 = od_load4(arow[0], cn, D), na1 = od_load4(arow[1], cn, D), nb = od_load4(brow, cn, D);
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, bv.x, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, bv.x, acc[1], 0, 0, 0);
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, bv.y, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, bv.y, acc[1], 0, 0, 0);
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, bv.z, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, bv.z, acc[1], 0, 0, 0);
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, bv.w, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, bv.w, acc[1], 0, 0, 0);
      a0 = na0; a1 = na1; bv = nb;
    }
    // keep what falls into the row's own window: column = position p (this lane), row = query
    if (p < P) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const int qi = i * 32 + od_acc_row(k, lh);
          const int ix = X - s_q[qi].qx0, iy = Y - s_q[qi].qy0;
          if (ix >= 0 && ix < WIN && iy >= 0 && iy < WIN) s_win[qi][iy * WIN + ix] = acc[i][k] * inv_sqrt_d;
        }
    }
  }
  __syncthreads();

  // blend and store: od_fwd_kernel's expression, channel order and runs along q (8 queries of a tile row)
  const size_t C = (size_t)Lo.L * NT;
  for (int i = threadIdx.x; i < NT * OD_TQ; i += 256) {
    const int tap = i / OD_TQ, qi = i % OD_TQ;
    const int y = ty0 + qi / OD_TW, x = tx0 + qi % OD_TW;
    if (y >= Lo.H || x >= Lo.W) continue;
    const BlendWeights w = blend_weights(s_q[qi].fx, s_q[qi].fy);
    const int a = tap / N1, bb = tap % N1;
    const float* c0 = &s_win[qi][bb * WIN + a];
    const float* c1 = c0 + WIN;
    out[((size_t)b * C + (size_t)l * NT + tap) * Q + (size_t)y * Lo.W + x] =
        blend4(c0[0], c0[1], c1[0], c1[1], w);
  }
}

// ---- backward: workgroup = tile, looping over the levels -------------------------------------------------------------------
// Wave w owns channels [64 w, 64 w + 64) of a 256-channel group.  dfmap1[64 x D] accumulates over the levels in MFMA
// accumulators (dC F2box, k = box position) and leaves in one plain store; per chunk of 64 box positions dF2box = dC^T F1
// (k = query, F1 held in registers) is quantised and added into acc element by element, in-map positions only.
constexpr int OD_BC = 64;               // box positions per chunk
constexpr int OD_LDC = OD_BC + 1;       // row stride of the dC image: row reads and column reads both spread over the banks

template <int R>
__global__ __launch_bounds__(256) void od_bwd_tile_kernel(OdLayout Lo, const float* __restrict__ f1t,
                                                          const float* __restrict__ pyr, const float* __restrict__ coords,
                                                          const float* __restrict__ grad, const OdTile* __restrict__ tab,
                                                          float* __restrict__ df1, long long* __restrict__ accp,
                                                          const int* __restrict__ shiftp, int accumulate,
                                                          float inv_sqrt_d) {
  constexpr int N1 = 2 * R + 1, WIN = 2 * R + 2, NT = N1 * N1;
  __shared__ float s_g[OD_TQ][NT + 1];
  __shared__ float s_dc[OD_TQ * OD_LDC];
  __shared__ OdTileQuery s_q[OD_TQ];
  __shared__ long long s_row[OD_BC];    // row of the chunk's position inside its level, -1: out of the map or past the box
  const int t = blockIdx.x, b = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 31, lh = lane >> 5;
  const int D = Lo.D, Q = Lo.Q;
  const int ntx = od_tiles_x(Lo.W), ty0 = (t / ntx) * OD_TH, tx0 = (t % ntx) * OD_TW;
  const OdTile* ent = tab + ((size_t)b * gridDim.x + t) * Lo.L;
  const float* zrow = pyr + (size_t)Lo.rows * D;
  const int shift = *shiftp;
  const bool scatter = shift != FIX_NONFINITE;
  const double scale = ldexp(1.0, scatter ? shift : 0);
  const size_t C = (size_t)Lo.L * NT;
  // this thread's query (rows of s_g it stages) and its coordinates
  const int myq = threadIdx.x & 63;
  const int my_y = ty0 + myq / OD_TW, my_x = tx0 + myq % OD_TW;
  const bool my_live = my_y < Lo.H && my_x < Lo.W;
  const int my_q = my_live ? my_y * Lo.W + my_x : 0;
  float cx = 0.f, cy = 0.f;
  if (threadIdx.x < OD_TQ) {
    cx = coords[((size_t)b * 2) * Q + my_q];
    cy = coords[((size_t)b * 2 + 1) * Q + my_q];
  }

  for (int dg = 0; dg < D; dg += 256) {
    const int d0 = dg + wv * 64;
    const bool wave_on = d0 < D;                 // wave-uniform: a wave past the last channel only builds dC
    const int dA = d0 + r, dB = d0 + 32 + r;     // this lane's two channels (column blocks 0 and 1)
    const int dAc = min(dA, D - 1), dBc = min(dB, D - 1);
    // F1 of the tile, B operand of dF2box = dC^T F1: k-step s covers queries 2 s + lh
    float f1r[32][2];
#pragma unroll
    for (int s = 0; s < 32; ++s) {
      const int qi = 2 * s + lh, y = ty0 + qi / OD_TW, x = tx0 + qi % OD_TW;
      const bool lv = y < Lo.H && x < Lo.W;
      const float* row = lv ? f1t + ((size_t)b * Q + (size_t)y * Lo.W + x) * D : zrow;
      const float va = row[dAc], vb = row[dBc];
      f1r[s][0] = dA < D ? va : 0.f;
      f1r[s][1] = dB < D ? vb : 0.f;
    }
    f32x16 g1[2][2];                             // dfmap1: [query block][channel block]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 16; ++k) g1[i][j][k] = 0.f;

    for (int l = 0; l < Lo.L; ++l) {
      const OdTile e = ent[l];
      if (e.bw == 0) continue;                   // block-uniform: od_bwd_kernel serves the level
      const int hl = Lo.h[l], wl = Lo.w[l];
      const float* lvl = pyr + ((size_t)Lo.prow[l] + (size_t)b * hl * wl) * D;
      long long* alvl = accp + ((size_t)Lo.prow[l] + (size_t)b * hl * wl) * D;
      const int P = e.bw * e.bh;
      __syncthreads();                           // the previous level's readers of s_g / s_q are done
      for (int i = threadIdx.x; i < NT * OD_TQ; i += 256) {
        const int tap = i / OD_TQ;               // i % 64 == myq
        s_g[myq][tap] = my_live ? grad[((size_t)b * C + (size_t)l * NT + tap) * Q + my_q] : 0.f;
      }
      if (threadIdx.x < OD_TQ) {
        OdTileQuery tq{-(1 << 30), -(1 << 30), 0.f, 0.f};
        if (my_live) {
          const Origin o = make_origin(cx, cy, l, R);
          tq = OdTileQuery{o.x0, o.y0, o.fx, o.fy};
        }
        s_q[threadIdx.x] = tq;
      }
      for (int p0 = 0; p0 < P; p0 += OD_BC) {
        __syncthreads();                         // s_g / s_q written; the previous chunk's readers of s_dc / s_row are done
        {
          // dC chunk: thread = (position pp, queries wv, wv + 4, ..)
          const int pp = threadIdx.x & 63, p = p0 + pp;
          const int py = p / e.bw, px = p - py * e.bw;
          const int X = e.bx0 + px, Y = e.by0 + py;
          const bool inmap = p < P && X >= 0 && X < wl && Y >= 0 && Y < hl;
          if (wv == 0) s_row[pp] = inmap ? (long long)Y * wl + X : -1;
#pragma unroll 4
          for (int qi = wv; qi < OD_TQ; qi += 4) {
            const OdTileQuery tq = s_q[qi];
            const int i = X - tq.qx0, j = Y - tq.qy0;
            float dc = 0.f;
            if (inmap && i >= 0 && i < WIN && j >= 0 && j < WIN) {
              const BlendWeights w = blend_weights(tq.fx, tq.fy);
              const float* G = s_g[qi];
              if (i < N1 && j < N1) dc += w.w00 * G[i * N1 + j];
              if (i >= 1 && j < N1) dc += w.w01 * G[(i - 1) * N1 + j];
              if (i < N1 && j >= 1) dc += w.w10 * G[i * N1 + j - 1];
              if (i >= 1 && j >= 1) dc += w.w11 * G[(i - 1) * N1 + j - 1];
              dc *= inv_sqrt_d;
            }
            s_dc[qi * OD_LDC + pp] = dc;
          }
        }
        __syncthreads();
        if (!wave_on) continue;
        const int nk = min(OD_BC, P - p0);       // live positions of the chunk; the rest of s_dc is 0
        // dfmap1 += dC F2box: k-step s covers positions 2 s + lh; the box rows are requested 8 steps ahead of their MFMAs.
        // The chunk's product has accumulators of its own: fp32 chains of <= 64 terms, folded into the tile's sum once
        // per chunk (the per-query kernel's chains are <= (2r+2)^2 terms for the same reason).
        f32x16 gc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 16; ++k) gc[i][j][k] = 0.f;
        for (int s0 = 0; s0 * 2 < nk; s0 += 8) {
          float fb[8][2];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const long long ro = s_row[2 * (s0 + u) + lh];
            const float* row = ro >= 0 ? lvl + (size_t)ro * D : zrow;
            const float va = row[dAc], vb = row[dBc];
            fb[u][0] = dA < D ? va : 0.f;
            fb[u][1] = dB < D ? vb : 0.f;
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int k = 2 * (s0 + u) + lh;
            const float a0 = s_dc[r * OD_LDC + k], a1 = s_dc[(32 + r) * OD_LDC + k];
            gc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, fb[u][0], gc[0][0], 0, 0, 0);
            gc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, fb[u][1], gc[0][1], 0, 0, 0);
            gc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, fb[u][0], gc[1][0], 0, 0, 0);
            gc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, fb[u][1], gc[1][1], 0, 0, 0);
          }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) g1[i][j] += gc[i][j];
        // dF2box = dC^T F1 for the chunk's two position blocks, then the fixed-point scatter
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          if (i * 32 >= nk) break;
          f32x16 g2[2];
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int k = 0; k < 16; ++k) g2[j][k] = 0.f;
#pragma unroll
          for (int s = 0; s < 32; ++s) {
            const float a = s_dc[(2 * s + lh) * OD_LDC + i * 32 + r];
            g2[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, f1r[s][0], g2[0], 0, 0, 0);
            g2[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, f1r[s][1], g2[1], 0, 0, 0);
          }
          if (scatter) {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
              const long long ro = s_row[i * 32 + od_acc_row(k, lh)];   // wave-uniform per lane half
              if (ro < 0) continue;
              long long* dst = alvl + (size_t)ro * D;
              if (dA < D && g2[0][k] != 0.f) fix_add(dst + dA, g2[0][k], scale);
              if (dB < D && g2[1][k] != 0.f) fix_add(dst + dB, g2[1][k], scale);
            }
          }
        }
      }
    }
    // dfmap1 of the tile: one plain store per element, live queries only
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int qi = i * 32 + od_acc_row(k, lh), y = ty0 + qi / OD_TW, x = tx0 + qi % OD_TW;
        if (!wave_on || y >= Lo.H || x >= Lo.W) continue;
        float* g = df1 + ((size_t)b * Q + (size_t)y * Lo.W + x) * D;
        if (dA < D) g[dA] = accumulate ? g[dA] + g1[i][0][k] : g1[i][0][k];
        if (dB < D) g[dB] = accumulate ? g[dB] + g1[i][1][k] : g1[i][1][k];
      }
  }
}

}  // namespace
