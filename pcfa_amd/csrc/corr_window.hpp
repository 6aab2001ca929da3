// The RAFT/GMA correlation window, stated once for every kernel that looks one up or has to know what a lookup touched:
// corr_lookup.hip, corr_lookup_conv.hip (windows of the 4x4-tiled slab, common.hpp), corr_ondemand.hip and
// corr_ondemand_tiled.hpp (windows computed on demand) and the tables of corr_pyramid.hip's sparse backward.
//   - All (2r+1)^2 taps of a (query, level) share one fractional offset, so a lookup is "fetch the (2r+2)^2 window at
//     floor(coords / 2^level) - r, blend it four ways"; the backward is the exact transpose.
//   - A slab window is fetched as PIECES: one piece = the 16 B (4 texels of one tile row) that one window row crosses in
//     one tile column.  Its LDS image holds the window with the sub-tile offset x0 & 3 removed.
//   - Which thread owns which piece, how a window's parameters reach it and how the 16 B are loaded is each kernel's own.
#pragma once
#include "common.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Pin a wave-uniform pointer into SGPRs.
template <typename T>
__device__ __forceinline__ T* scalar_ptr(T* p) {
  const unsigned long long u = reinterpret_cast<unsigned long long>(p);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
  return reinterpret_cast<T*>(((unsigned long long)hi << 32) | lo);
}

// ---- where a window starts -------------------------------------------------------------------------------------------
// The texel of coordinate c at `level`: coords / 2**level (exact power-of-two scaling), floor; the clamp keeps the
// conversion defined for huge coordinates and sends NaN to -1e8.  Also the tables' "which texel can a window have touched".
__device__ __forceinline__ int window_texel(float c, int level) {
  return (int)fminf(fmaxf(floorf(c * (1.0f / (float)(1 << level))), -1.0e8f), 1.0e8f);
}

struct Origin {
  int x0, y0;    // window origin (texels, level coordinates)
  float fx, fy;  // shared bilinear fractions
};

__device__ __forceinline__ Origin make_origin(float cx, float cy, int level, int R) {
  const float inv = 1.0f / (float)(1 << level);
  const float xl = cx * inv, yl = cy * inv;
  Origin o;
  o.fx = xl - floorf(xl);
  o.fy = yl - floorf(yl);
  o.x0 = window_texel(cx, level) - R;
  o.y0 = window_texel(cy, level) - R;
  return o;
}

// The origin folded onto the level (hl rows, tw tile columns): any window that misses the level keeps missing it, and
// the origin fits 16 bits with a bias of 16.  A dead query collapses onto the first row past the level's tile rows, so
// that every one of its pieces is invalid.
__device__ __forceinline__ Origin clamp_origin(Origin o, bool live, int hl, int tw) {
  const int th4 = ((hl + 3) >> 2) << 2;
  o.x0 = min(max(o.x0, -16), 4 * tw);
  o.y0 = live ? min(max(o.y0, -16), th4) : th4;
  return o;
}

// ---- the pieces of a slab window and its LDS image ----------------------------------------------------------------------
constexpr int RS = 20;  // LDS row stride (floats): 4 pad + 16; window texel (r, c) sits at r*RS + 4 + c

// QB = queries (= windows) per workgroup; the fields that depend on it are corr_lookup.hip's work split.
template <int R, int QB>
struct Geo {
  static_assert(QB == 64 || QB == 32 || QB == 16, "lane % QB = query needs QB to divide the wave");
  static constexpr int N1 = 2 * R + 1;                      // taps per axis
  static constexpr int WIN = 2 * R + 2;                     // window texels per axis
  static constexpr int RPW = 64 / QB;                       // window rows (phase B) per wave
  static constexpr int NW = (N1 + RPW - 1) / RPW;           // waves per workgroup
  static constexpr int TXN = ((WIN + 2) >> 2) + 1;          // tile columns a window can cross
  static constexpr int PIECES = WIN * TXN;                  // 16-B pieces per window
  static constexpr int NP = (QB * PIECES + NW * 64 - 1) / (NW * 64);  // piece wave-instructions per wave
  static constexpr bool FULL = QB * PIECES == NW * NP * 64; // every piece slot of every wave is a real piece
  static constexpr int WS = WIN * RS + 4;                   // floats per window image; WS/4 odd -> the b128 accesses
                                                            // of 16 consecutive windows hit 16 distinct bank groups
  static constexpr int NRD = (WIN + 3) / 4;                 // b128 accesses per window row
  static constexpr int LDS_FLOATS = QB * WS + 4;            // + a 16-B dump slot for lanes without a piece
};

// Window row rr, tile column tx of the window at the clamped origin (x0, y0).  piece_geometry gives goff and lds in
// floats, relative to the level's first texel and to the window's image; a kernel rebases both onto its own slab
// pointer and LDS array (and replaces the goff of a piece that is not needed: it is no address inside the level).
struct Piece {
  unsigned goff;  // of the piece's 16 B in the pyramid
  unsigned lds;   // of the piece's first texel in the window image (unaligned by the window's x0 & 3)
  int mask;       // bit e (< 4): texel e of the piece is a window texel inside the level; bit 4 ("need"): the
                  // piece holds texels of the level at all (else: zeros / nothing to add)
  __device__ __forceinline__ bool need() const { return (mask & 16) != 0; }
};

__device__ __forceinline__ Piece piece_geometry(int x0, int y0, int rr, int tx, int hl, int wl, int tw, int WIN) {
  const int ox = x0 & 3, y = y0 + rr, gtx = (x0 >> 2) + tx;
  const bool need = (unsigned)y < (unsigned)hl && (unsigned)gtx < (unsigned)tw && 4 * tx < ox + WIN;
  const int c0 = 4 * tx - ox, gx0 = 4 * gtx;  // window column / level x of the piece's first texel
  Piece pc;
  int texels = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if ((unsigned)(c0 + e) < (unsigned)WIN && gx0 + e < wl) texels |= 1 << e;
  pc.mask = texels | (need ? 16 : 0);   // need goes in last: a caller that only asks need() never builds the texel bits
  pc.goff = ((((unsigned)y >> 2) * (unsigned)tw + (unsigned)gtx) << 4) + (((unsigned)y & 3u) << 2);
  pc.lds = (unsigned)(rr * RS + 4 + 4 * tx - ox);
  return pc;
}

// ---- the blend and its transpose ---------------------------------------------------------------------------------------
struct BlendWeights {
  float w00, w01, w10, w11;
};
__device__ __forceinline__ BlendWeights blend_weights(float fx, float fy) {
  BlendWeights w;
  w.w00 = (1.f - fx) * (1.f - fy);
  w.w01 = fx * (1.f - fy);
  w.w10 = (1.f - fx) * fy;
  w.w11 = fx * fy;
  return w;
}
// one tap from window texels (y, x), (y, x+1), (y+1, x), (y+1, x+1)
__device__ __forceinline__ float blend4(float t00, float t01, float t10, float t11, const BlendWeights& w) {
  return t00 * w.w00 + t01 * w.w01 + t10 * w.w10 + t11 * w.w11;
}

// Row `row` (< N1) of the window's gradient image, NRD * 4 floats, from the tap gradients gc[a] = g(a, row) and
// gp[a] = g(a, row - 1) (zeros for row 0), a = x offset:
//   d window[r][c] = w00 g[c][r] + w01 g[c-1][r] + w10 g[c][r-1] + w11 g[c-1][r-1]   (g = 0 outside 0..2r)
template <int N1, int NRD>
__device__ __forceinline__ void window_grad_row(const float (&gc)[N1], const float (&gp)[N1], const BlendWeights& w,
                                                float (&d)[NRD * 4]) {
#pragma unroll
  for (int c = 0; c < NRD * 4; ++c) {
    float s = 0.f;
    if (c < N1) s = gc[c] * w.w00;
    if (c >= 1 && c <= N1) s = fmaf(gc[c - 1], w.w01, s);
    if (c < N1) s = fmaf(gp[c], w.w10, s);
    if (c >= 1 && c <= N1) s = fmaf(gp[c - 1], w.w11, s);
    d[c] = s;
  }
}
// The window's last row, N1: only the row above contributes (gc = the tap gradients of row N1 - 1).
template <int N1, int NRD>
__device__ __forceinline__ void window_grad_last_row(const float (&gc)[N1], const BlendWeights& w, float (&d)[NRD * 4]) {
#pragma unroll
  for (int c = 0; c < NRD * 4; ++c) {
    float s = 0.f;
    if (c < N1) s = gc[c] * w.w10;
    if (c >= 1 && c <= N1) s = fmaf(gc[c - 1], w.w11, s);
    d[c] = s;
  }
}

// A piece of the gradient image (e0..e3) added into a piece of dpyr (t).  Image cells outside the window's columns were
// never written; texels beyond the level width stay zero.
__device__ __forceinline__ f32x4 piece_add(f32x4 t, float e0, float e1, float e2, float e3, int mask) {
  t.x += (mask & 1) ? e0 : 0.f;
  t.y += (mask & 2) ? e1 : 0.f;
  t.z += (mask & 4) ? e2 : 0.f;
  t.w += (mask & 8) ? e3 : 0.f;
  return t;
}

}  // namespace
