// What the dense GEMM cores share (corr_pyramid.hip: fp32 MFMA; gemm_bf16x3.hip: split-bf16 MFMA): the 128x128 block
// tile of 4 waves (2x2) with 2x2 accumulators of a 32x32 MFMA each, its epilogues, and the ordered split-K reduction.
// The C/D register map of a 32x32 MFMA does not depend on the input type (v_mfma_f32_32x32x2_f32 and
// v_mfma_f32_32x32x16_bf16 alike: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)), so one statement of
// the epilogues serves both.
#pragma once
#include "common.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128, BN = 128;

// POOL (correlation pyramid forward only): the GEMM runs over the level-0 columns [0, S0) and the tail columns
// [off_tail, slab) (levels >= 3 and the zero tile, taken from f2ext as before); levels 1 and 2 are average-pooled from
// the level-0 accumulators in the epilogue, the way the reference pools the correlation volume
// (models/raft/corr.py:24-27: F.avg_pool2d of the level below) -- 24 % fewer MFMAs than multiplying against the
// pooled copies of fmap2, and the pooled values round like the reference's.  Needs W % 16 == 0 (no x padding inside
// the tiles of levels 1 and 2) and L >= 3; the caller checks.
// Every float of a slab has exactly one store: the level-0 columns and the tail from the GEMM itself, a texel of levels
// 1 and 2 from the level-0 tile it is pooled from (zero where the texel lies in a pad row of its level), and the pad rows
// of the last tile row of levels 1 and 2 that no level-0 tile pools into from the last level-0 tile row.  A level-0 tile
// row below the last tile row of level 1 or 2 (H % 8 == 1, H % 16 in {1, 2, 3}) stores nothing there.
// (tests/pyramid.py: store_map restates these stores; change both together.)
struct PoolArgs {
  int nb0;        // N-blocks (of BN columns) covering the level-0 columns
  int S0;         // level-0 columns (tiles x 16)
  int off_tail;   // first tail column
  int tw0, tiles0;
  int th0;        // level-0 tile rows
  int off1, tw1, h1, w1;
  int off2, tw2, h2, w2;
};
constexpr int SC = BN + 4;   // row stride of the epilogue image of the C tile

// The PoolArgs of a pyramid layout; false: the layout does not fit the pooled epilogue.
inline bool make_pool_args(const PyrLayout& P, PoolArgs& pa) {
  pa.tw0 = P.tw[0];
  pa.tiles0 = ((P.h[0] + 3) / 4) * P.tw[0];
  pa.th0 = (P.h[0] + 3) / 4;
  pa.S0 = pa.tiles0 * 16;
  pa.nb0 = pcfa_cdiv(pa.S0, BN);
  pa.off_tail = P.L > 3 ? P.off[3] : P.zero;
  pa.off1 = P.off[1]; pa.tw1 = P.tw[1]; pa.h1 = P.h[1]; pa.w1 = P.w[1];
  pa.off2 = P.off[2]; pa.tw2 = P.tw[2]; pa.h2 = P.h[2]; pa.w2 = P.w[2];
  return pa.S0 == P.off[1] && pa.off_tail % 16 == 0 && pa.off_tail <= P.slab;
}

// Levels 1 and 2 of the pooled epilogue from the image sC of a level-0 block tile: thread = (query row, 4x4 tile); sums
// in avg_pool2d's window order, one division by 4 each.  A level-0 tile row with another below it lies inside the tile
// rows of levels 1 and 2, and every row of those it pools into has its own level-0 tiles.  LAST: the block may hold
// tiles of the last level-0 tile row.  That row stores only where its tile row of level 1 / 2 exists, and it owns the
// rows of that tile row below its own (pad rows: no level-0 tile pools into them), which it zeroes.
template <bool LAST>
__device__ __forceinline__ void gemm_tile_pool_levels(const float* sC, float* __restrict__ C, int M, long long ldc, int m0,
                                                      int n0, const PoolArgs& pool) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < BM * (BN / 16) / 256; ++k) {
    const int item = tid + 256 * k, row = item >> 3, t = item & 7;
    const int T0 = n0 / 16 + t;
    if (m0 + row >= M || T0 >= pool.tiles0) continue;
    const int ty = T0 / pool.tw0, tx = T0 - ty * pool.tw0;
    float v[4][4];
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      const float4 q4 = *reinterpret_cast<const float4*>(&sC[row * SC + 16 * t + 4 * y]);
      v[y][0] = q4.x; v[y][1] = q4.y; v[y][2] = q4.z; v[y][3] = q4.w;
    }
    float* crow = C + (long long)(m0 + row) * ldc;
    float* d1 = crow + pool.off1 + ((ty >> 1) * pool.tw1 + (tx >> 1)) * 16 + 2 * (ty & 1) * 4 + 2 * (tx & 1);
    float* d2 = crow + pool.off2 + ((ty >> 2) * pool.tw2 + (tx >> 2)) * 16 + (ty & 3) * 4 + (tx & 3);
    const bool last = LAST && ty == pool.th0 - 1;
    const bool in1 = !last || (ty >> 1) < ((pool.h1 + 3) >> 2), in2 = !last || (ty >> 2) < ((pool.h2 + 3) >> 2);
    float l1[2][2];
#pragma unroll
    for (int Y = 0; Y < 2; ++Y) {
#pragma unroll
      for (int X = 0; X < 2; ++X) {
        const float sum = ((v[2 * Y][2 * X] + v[2 * Y][2 * X + 1]) + v[2 * Y + 1][2 * X]) + v[2 * Y + 1][2 * X + 1];
        l1[Y][X] = (2 * ty + Y < pool.h1 && 2 * tx + X < pool.w1) ? sum * 0.25f : 0.f;
      }
      if (in1) *reinterpret_cast<float2*>(d1 + 4 * Y) = make_float2(l1[Y][0], l1[Y][1]);
    }
    const float sum2 = ((l1[0][0] + l1[0][1]) + l1[1][0]) + l1[1][1];
    if (in2) *d2 = (ty < pool.h2 && tx < pool.w2) ? sum2 * 0.25f : 0.f;
    if (last) {
      if (in1 && !(ty & 1)) {   // rows 2, 3 of this level-1 tile row
        *reinterpret_cast<float2*>(d1 + 8) = make_float2(0.f, 0.f);
        *reinterpret_cast<float2*>(d1 + 12) = make_float2(0.f, 0.f);
      }
      if (in2)                  // the rows below in this level-2 tile row
        for (int y = (ty & 3) + 1; y < 4; ++y) d2[4 * (y - (ty & 3))] = 0.f;
    }
  }
}

// Epilogue of one 128x128 block tile at (m0, n0): C = acc / div.  `smem` (BM * SC floats, free of readers: the main
// loop ended on a barrier) is used only by the pooled form.
// The reference divides by sqrt(D); when that is a power of two (D = 256 -> 16) multiplying by its reciprocal
// is the same fp32 result and saves a division sequence per output element.
template <bool POOL>
__device__ __forceinline__ void gemm_tile_epilogue(const f32x16 (&acc)[2][2], float* smem,
                                                   float* __restrict__ C, int M, int N, long long ldc, int m0, int n0,
                                                   float div, bool pooled, const PoolArgs& pool) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int l31 = lane & 31, lh = lane >> 5;
  int dexp;
  const bool pow2 = frexpf(div, &dexp) == 0.5f;
  const float rdiv = 1.0f / div;
  if (POOL && pooled) {
    // ---- C tile -> LDS ----
    float* sC = smem;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          sC[row * SC + wc * 64 + j * 32 + l31] = pow2 ? acc[i][j][r] * rdiv : acc[i][j][r] / div;
        }
    __syncthreads();
    const int tid = threadIdx.x;
    // level 0: rows of 512 B, 16-B stores
#pragma unroll
    for (int k = 0; k < BM * BN / 4 / 256; ++k) {
      const int idx = tid + 256 * k, row = idx >> 5, c4 = (idx & 31) * 4;
      if (m0 + row < M && n0 + c4 < N)
        *reinterpret_cast<float4*>(&C[(long long)(m0 + row) * ldc + n0 + c4]) =
            *reinterpret_cast<const float4*>(&sC[row * SC + c4]);
    }
    // levels 1 and 2 (workgroup-uniform choice: does this block hold tiles of the last level-0 tile row?)
    if ((n0 / 16 + BN / 16 - 1) / pool.tw0 < pool.th0 - 1) gemm_tile_pool_levels<false>(sC, C, M, ldc, m0, n0, pool);
    else gemm_tile_pool_levels<true>(sC, C, M, ldc, m0, n0, pool);
    return;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wc * 64 + j * 32 + l31;
      if (col >= N) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (row < M) C[(long long)row * ldc + col] = pow2 ? acc[i][j][r] * rdiv : acc[i][j][r] / div;
      }
    }
}

// XCD-aware tile order (cdna_hip_programming.md T1, bijective form): workgroups are dealt round-robin over the 8
// XCDs, so consecutive linear ids land on different L2s; remapped, every XCD walks a contiguous band of tile rows
// and re-reads its A band / the streamed B tiles from its own L2.  Speed only -- any placement is correct.
__device__ __forceinline__ void gemm_tile_xcd_order(int& by, int& bx) {
#ifndef PCFA_GEMM_NO_XCD
  const int nx = gridDim.x, nwg = nx * gridDim.y;
  const int orig = by * nx + bx, xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
  const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
  by = wg / nx;
  bx = wg - by * nx;
#endif
}

// out[i] = sum_s partial[s][i]  (fixed order -> deterministic).  No scaling:
// the split GEMMs already divided every partial by sqrt(D).
__global__ void splitk_reduce_kernel(const float* __restrict__ part, float* __restrict__ out,
                                     long long n, int splits, long long ss) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    float s = part[i];
    for (int k = 1; k < splits; ++k) s += part[(long long)k * ss + i];
    out[i] = s;
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
