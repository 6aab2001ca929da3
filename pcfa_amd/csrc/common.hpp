// Shared host/device helpers for libpcfa_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "../../include/pcfa_hip.h"

#define PCFA_WAVE 64

#define PCFA_LAUNCH_CHECK()                          \
  do {                                               \
    hipError_t _e = hipGetLastError();               \
    if (_e != hipSuccess) return (int)_e;            \
  } while (0)

// Pyramid layout shared by every corr kernel (passed by value as a kernel arg).
//
// One row ("slab") of the pyramid matrix per query.  Inside a slab every level is stored as
// 4x4-texel TILES (64 B = one HBM/L2 sector each), tiles row-major, texels row-major inside a
// tile:   idx(l, y, x) = off[l] + ((y>>2)*tw[l] + (x>>2))*16 + (y&3)*4 + (x&3).
// A (2r+2)^2 lookup window then touches ~11 sectors instead of ~16-20 with plain rows, and a
// wave fetches a whole window with ONE 16-B-per-lane load (lane = tile row).  Levels are padded
// to whole tiles; pad texels and the closing zero tile hold +0 in every slab the forward builds: the GEMM multiplies zero
// columns of f2ext there, and the pooled epilogue (gemm_tile.hpp) stores zeros into the pad rows of levels 1 and 2.
struct PyrLayout {
  int L;
  int h[PCFA_MAX_LEVELS];
  int w[PCFA_MAX_LEVELS];
  int tw[PCFA_MAX_LEVELS];   // tiles per tile-row
  int off[PCFA_MAX_LEVELS];  // floats, multiple of 16
  int zero;                  // offset of a tile that is always 0 (f2ext has zero columns there)
  int slab;                  // floats per query row, multiple of 16
};

static inline bool pcfa_make_layout(PyrLayout& P, int H, int W, int L) {
  if (L < 1 || L > PCFA_MAX_LEVELS || H < 1 || W < 1) return false;
  P.L = L;
  long long off = 0;
  int h = H, w = W;
  for (int l = 0; l < PCFA_MAX_LEVELS; ++l) {
    if (l < L) {
      P.h[l] = h;
      P.w[l] = w;
      P.tw[l] = (w + 3) / 4;
      P.off[l] = (int)off;
      off += (long long)((h + 3) / 4) * ((w + 3) / 4) * 16;
      h /= 2;
      w /= 2;
    } else {
      P.h[l] = 0;
      P.w[l] = 0;
      P.tw[l] = 0;
      P.off[l] = (int)off;
    }
  }
  P.zero = (int)off;  // one all-zero tile closes every slab (out-of-window lanes load it branch-free)
  off += 16;
  if (off > 0x7fffffffLL / 4) return false;
  P.slab = (int)off;
  return true;
}

#if defined(__HIPCC__)
__host__ __device__
#endif
static inline int pcfa_tiled_index(const PyrLayout& P, int l, int y, int x) {
  return P.off[l] + (((y >> 2) * P.tw[l] + (x >> 2)) << 4) + ((y & 3) << 2) + (x & 3);
}

static inline int pcfa_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// ---- XCD-aware workgroup -> work-item maps -----------------------------------------------------------------------
// Workgroups are dealt to the 8 XCDs round-robin by their linear id and every XCD has its own 4 MB L2.  A kernel whose
// neighbouring work items share data (halos, a weight slice) therefore launches a 1-D grid and lets XCD k = id & 7 own a
// contiguous sub-rectangle of its (x, y) item space: a x b = 8 sub-rectangles, a splits x, b splits y.  Items past the end
// of a sub-rectangle are dead workgroups that return at once (the grid is padded to 8 * ceil(gx / a) * ceil(gy / b)).
// Measured on the PWC cost volume (1-D form, spatial_corr.hip): L2 misses 30.1 -> 10.3 MB (forward), 137.6 -> 35.9 MB (backward).
struct PcfaXcdMap {
  int a, b;        // sub-rectangles along x / y (a * b == 8); a == 0: identity (plain 2-D grid)
  int gx, gy;      // item space
};
static inline unsigned pcfa_xcd_grid(const PcfaXcdMap& m) {
  return 8u * (unsigned)pcfa_cdiv(m.gx, m.a) * (unsigned)pcfa_cdiv(m.gy, m.b);
}
// a, b minimising the per-XCD footprint x_bytes / a + y_bytes / b (x_bytes: data that follows x, e.g. the input planes;
// y_bytes: data that follows y, e.g. the weights), with a <= gx and b <= gy
static inline PcfaXcdMap pcfa_xcd_pick(int gx, int gy, double x_bytes, double y_bytes) {
  PcfaXcdMap best{8, 1, gx, gy};
  double cost = -1.0;
  for (int a = 8; a >= 1; a >>= 1) {
    const int b = 8 / a;
    if (a > gx || b > gy) continue;
    const double c = x_bytes / a + y_bytes / b;
    if (cost < 0.0 || c < cost) {
      cost = c;
      best.a = a;
      best.b = b;
    }
  }
  if (cost < 0.0) best.a = 0;   // fewer than 8 items either way: nothing to place
  return best;
}
#if defined(__HIPCC__)
// (x, y) of this workgroup under map m from the 1-D id `lin`; false: dead workgroup (return before any barrier).
// Inside an XCD x runs fastest: consecutive workgroups of one XCD share their y data (the weight slice) in time.
__device__ __forceinline__ bool pcfa_xcd_item(const PcfaXcdMap& m, int lin, int& x, int& y) {
  const int k = lin & 7, r = lin >> 3;
  const int cx = (m.gx + m.a - 1) / m.a, cy = (m.gy + m.b - 1) / m.b;
  const int yy = r / cx, xx = r - yy * cx;
  x = (k % m.a) * cx + xx;
  y = (k / m.a) * cy + yy;
  return x < m.gx && y < m.gy && yy < cy;
}

// maximum of m over a 256-thread workgroup, on every thread (red: 4 floats of LDS)
__device__ __forceinline__ float block_max_256(float m, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return m;
}

// Zero fill of N float buffers in one launch, grid-stride, four floats per thread and step (one 16-byte store where the
// buffer is aligned and four floats remain).  Any 1-D grid of any block size.  A kernel, not hipMemsetAsync: inside torch's
// stream capture the memset node was not replayed with the graph (stale gradients accumulated from replay to replay).
template <int N>
struct ZeroSpans {
  float* p[N];
  long long n[N];
};
template <int N>
__global__ void zero_fill_kernel(ZeroSpans<N> z) {
  const long long step = (long long)gridDim.x * blockDim.x * 4;
  for (int b = 0; b < N; ++b) {
    float* p = z.p[b];
    const long long n = z.n[b];
    for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += step) {
      if (i + 3 < n && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        *reinterpret_cast<float4*>(p + i) = make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        for (long long k = i; k < n && k < i + 4; ++k) p[k] = 0.f;
      }
    }
  }
}
#endif

// ---- measurement hook -----------------------------------------------------------------------------------
// pcfa_timing_arm(start, stop, nth) (include/pcfa_hip.h) queues a pair of caller-owned hipEvents for the nth kernel
// this thread launches next; that kernel is then dispatched with hipExtLaunchKernel, which attaches the events to
// its dispatch packet (begin/end timestamps of the kernel itself, no barrier packets).  Nothing is armed in
// normal operation and every launch below is a plain hipLaunchKernelGGL.
struct PcfaArmed {
  hipEvent_t start, stop;
  int nth;
};
struct PcfaTimingState {
  PcfaArmed q[8];
  int n = 0;
  int launched = 0;
};
PcfaTimingState& pcfa_timing_state();  // thread-local, defined in attack_math.hip

template <typename K, typename... Args>
inline void pcfa_launch(K kernel, dim3 grid, dim3 block, size_t shmem, hipStream_t s, Args... args) {
  PcfaTimingState& t = pcfa_timing_state();
  if (t.n > 0) {
    const int idx = t.launched++;
    for (int i = 0; i < t.n; ++i)
      if (t.q[i].nth == idx) {
        const PcfaArmed a = t.q[i];
        t.q[i] = t.q[--t.n];
        hipExtLaunchKernelGGL(kernel, grid, block, shmem, s, a.start, a.stop, 0, args...);
        return;
      }
  }
  hipLaunchKernelGGL(kernel, grid, block, shmem, s, args...);
}
