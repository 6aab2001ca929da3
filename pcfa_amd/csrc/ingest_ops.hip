// Dataset ingest for gfx950: the per-pixel half of reading a Sintel / KITTI-15 PNG, the mirror image of artefact_ops.hip.
//
// The host does what is serial by nature (file read, zlib inflate: helper_functions/png.py); the device undoes the
// scanline filters and unpacks the samples into the planar fp32 tensors the attack works on.
//
// Replaces (reference paths):
//   PIL's / OpenCV's decoders behind read_gen, readFlowKITTI     helper_functions/frame_utils.py
//   uint8 -> float, permute, tile / drop alpha, enforce_dimensions  helper_functions/datasets.py (FlowDataset.__getitem__)
//
// pcfa_png_unfilter.  Reconstruction (PNG specification, "Filter types") of byte x of row y needs the bytes one pixel to
// the left, one row up and up-left, so the work is a skewed wavefront: thread r owns row r of a band of at most 1024 rows
// and at step s reconstructs pixel s - r.  `left` and `upper-left` stay in registers; `up` comes from the slot that row
// r - 1 wrote one step earlier, a double-buffered LDS array of 8 bytes per row and half: step s reads half (s - 1) & 1 and
// writes half s & 1, so ONE workgroup barrier per step orders both hand-overs.  Every thread of the workgroup runs the
// same W + rows - 1 trips and meets every barrier; there is no atomic, no spin-wait and only one workgroup per launch.
// A taller image runs as bands, one launch after the other on the stream: row 0 of a later band reads its `up` pixels from
// `raw`, which the previous launch completed.  A thread fetches its filtered pixel (and row 0 its `up` pixel) one step
// before it needs it, so the chain left -> pixel of a step never starts with a load.  The predictors are computed
// branch-free and selected by the row's filter type: the rows of a wave carry different types.
//
// pcfa_samples_to_planar.  Fully parallel: a thread converts four neighbouring output pixels of one row for all three
// planes and stores one 16-byte piece per plane where the piece is aligned and whole, single floats otherwise (same values).
#include "common.hpp"

namespace {

constexpr int UNF_MAX_ROWS = 1024;     // rows per band = threads per workgroup at most
constexpr int PLANAR_THREADS = 256;
constexpr int PLANAR_MAX_BLOCKS = 2048;   // grid-stride beyond

typedef unsigned long long px_t;   // one pixel's bytes, byte c in bits [8c, 8c + 8); bpp <= 6

template <int BPP>
__device__ __forceinline__ px_t load_px(const unsigned char* p) {
  px_t v = 0;
#pragma unroll
  for (int c = 0; c < BPP; ++c) v |= (px_t)p[c] << (8 * c);
  return v;
}

template <int BPP>
__device__ __forceinline__ void store_px(unsigned char* p, px_t v) {
#pragma unroll
  for (int c = 0; c < BPP; ++c) p[c] = (unsigned char)(v >> (8 * c));
}

// Recon(x) = Filt(x) + predictor, modulo 256, per byte; a = left, b = up, c = upper-left (each the byte of the same channel).
// The rows of one wave carry different filter types, so the predictor is picked by four masks (all ones for the row's own
// type, none set for type 0) instead of a branch per type.
struct FilterMasks {
  int sub, up, avg, paeth;
};
__device__ __forceinline__ FilterMasks filter_masks(unsigned ft) {
  return FilterMasks{-(int)(ft == 1u), -(int)(ft == 2u), -(int)(ft == 3u), -(int)(ft == 4u)};
}

template <int BPP>
__device__ __forceinline__ px_t reconstruct(const FilterMasks m, px_t filt, px_t left, px_t up, px_t upleft) {
  px_t out = 0;
#pragma unroll
  for (int k = 0; k < BPP; ++k) {
    const int f = (int)((filt >> (8 * k)) & 255), a = (int)((left >> (8 * k)) & 255);
    const int b = (int)((up >> (8 * k)) & 255), c = (int)((upleft >> (8 * k)) & 255);
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);   // |p - a|, |p - b|, |p - c| with p = a + b - c
    const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    const int pred = (a & m.sub) | (b & m.up) | (((a + b) >> 1) & m.avg) | (paeth & m.paeth);
    out |= (px_t)((f + pred) & 255) << (8 * k);
  }
  return out;
}

// One band: rows y0 .. y0 + rows - 1, ONE workgroup of at least `rows` threads (a multiple of 64).  `raw` is read (the row
// above the band) as well as written, hence no __restrict__.
template <int BPP>
__global__ __launch_bounds__(UNF_MAX_ROWS) void png_unfilter_kernel(const unsigned char* filtered, unsigned char* raw,
                                                                    int y0, int rows, int W) {
  __shared__ px_t slot[2][UNF_MAX_ROWS];
  const int r = threadIdx.x;
  const bool mine = r < rows;
  const long long row_bytes = (long long)W * BPP;
  const long long y = y0 + (mine ? r : 0);
  const unsigned char* src = filtered + y * (row_bytes + 1);
  unsigned char* dst = raw + y * row_bytes;
  // only row 0 of a band that is not the image's first reads the row above from memory
  const unsigned char* above = (r == 0 && y0 > 0) ? raw + (long long)(y0 - 1) * row_bytes : nullptr;
  const FilterMasks masks = filter_masks(mine ? src[0] : 0u);
  src += 1;
  px_t left = 0, upleft = 0;
  // The filtered pixel is fetched one step before its use, by EVERY thread in EVERY step from an address that depends on
  // (s, r) alone (clamped into the row): the load sits outside all divergent control flow, at the head of the step, and
  // the step's own arithmetic covers its latency (the compiler retires it before the step's barrier).  Row 0's `up` pixel
  // from memory is fetched the same way, but only where a band has a row above it.
  px_t next = load_px<BPP>(src);
  px_t up_next = above ? load_px<BPP>(above) : 0;
  const int steps = W + rows - 1;                    // the same for every thread: nobody leaves before the last barrier
  for (int s = 0; s < steps; ++s) {
    const int x = s - r;
    const int xn = min(max(x + 1, 0), W - 1);
    const px_t filt = next;
    next = load_px<BPP>(src + (long long)xn * BPP);
    px_t up = up_next;
    if (above) up_next = load_px<BPP>(above + (long long)xn * BPP);
    if (mine && x >= 0 && x < W) {
      if (r > 0) up = slot[(s & 1) ^ 1][r - 1];
      const px_t px = reconstruct<BPP>(masks, filt, left, up, upleft);
      slot[s & 1][r] = px;
      store_px<BPP>(dst + (long long)x * BPP, px);
      left = px;
      upleft = up;
    }
    __syncthreads();
  }
}

template <int BPP>
int unfilter_bands(const unsigned char* filtered, unsigned char* raw, int H, int W, hipStream_t s) {
  for (int y0 = 0; y0 < H; y0 += UNF_MAX_ROWS) {
    const int rows = H - y0 < UNF_MAX_ROWS ? H - y0 : UNF_MAX_ROWS;
    pcfa_launch(png_unfilter_kernel<BPP>, dim3(1), dim3(pcfa_cdiv(rows, PCFA_WAVE) * PCFA_WAVE), 0, s, filtered, raw, y0,
                rows, W);
    PCFA_LAUNCH_CHECK();
  }
  return PCFA_OK;
}

// ---------------------------------------------------------------- samples -> planar fp32
enum { KIND_RGB8 = 0, KIND_GREY8 = 1, KIND_RGBA8 = 2, KIND_KITTI_FLOW16 = 3 };

// the three plane values of source pixel p (its first byte)
template <int KIND>
__device__ __forceinline__ void unpack(const unsigned char* p, float v[3]) {
  if (KIND == KIND_GREY8) {
    v[0] = v[1] = v[2] = (float)p[0];
  } else if (KIND == KIND_KITTI_FLOW16) {   // big-endian 16-bit R, G, B: (R - 2^15) / 64, (G - 2^15) / 64, B -- all exact in fp32
    const int R = (p[0] << 8) | p[1], G = (p[2] << 8) | p[3], B = (p[4] << 8) | p[5];
    v[0] = (float)(R - 32768) * (1.f / 64.f);
    v[1] = (float)(G - 32768) * (1.f / 64.f);
    v[2] = (float)B;
  } else {   // RGB, RGBA (alpha dropped)
    v[0] = (float)p[0];
    v[1] = (float)p[1];
    v[2] = (float)p[2];
  }
}

template <int KIND, int BPP>
__global__ __launch_bounds__(PLANAR_THREADS) void samples_to_planar_kernel(const unsigned char* __restrict__ raw, int H, int W,
                                                                            float* __restrict__ out, int Hp, int Wp) {
  const long long gpr = (Wp + 3) / 4;            // groups of four output pixels per row
  const long long groups = gpr * Hp;
  const long long plane = (long long)Hp * Wp;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += step) {
    const long long y = g / gpr;
    const int x0 = (int)(g - y * gpr) * 4;
    const int n = Wp - x0 < 4 ? Wp - x0 : 4;
    float v[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k][0] = v[k][1] = v[k][2] = 0.f;          // outside the source: F.pad's constant 0
      if (k < n && y < H && x0 + k < W) unpack<KIND>(raw + (y * W + x0 + k) * BPP, v[k]);
    }
    float* o = out + y * Wp + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* oc = o + c * plane;
      if (n == 4 && (reinterpret_cast<uintptr_t>(oc) & 15) == 0) {
        *reinterpret_cast<float4*>(oc) = make_float4(v[0][c], v[1][c], v[2][c], v[3][c]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < n) oc[k] = v[k][c];
      }
    }
  }
}

template <int KIND, int BPP>
void planar_launch(const unsigned char* raw, int H, int W, float* out, int Hp, int Wp, hipStream_t s) {
  const long long groups = (long long)((Wp + 3) / 4) * Hp;
  const long long blocks = (groups + PLANAR_THREADS - 1) / PLANAR_THREADS;
  pcfa_launch(samples_to_planar_kernel<KIND, BPP>, dim3((unsigned)(blocks < PLANAR_MAX_BLOCKS ? blocks : PLANAR_MAX_BLOCKS)),
              dim3(PLANAR_THREADS), 0, s, raw, H, W, out, Hp, Wp);
}

}  // namespace

extern "C" int pcfa_png_unfilter(const unsigned char* filtered, unsigned char* raw, int H, long long row_bytes, int bpp,
                                 void* stream) {
  if (!filtered || !raw || H < 1 || row_bytes < 1 || (bpp != 1 && bpp != 3 && bpp != 4 && bpp != 6) || row_bytes % bpp != 0 ||
      row_bytes / bpp > 0x7fffffffLL - UNF_MAX_ROWS)
    return PCFA_ERR_INVALID_ARG;
  const int W = (int)(row_bytes / bpp);
  hipStream_t s = (hipStream_t)stream;
  switch (bpp) {
    case 1: return unfilter_bands<1>(filtered, raw, H, W, s);
    case 3: return unfilter_bands<3>(filtered, raw, H, W, s);
    case 4: return unfilter_bands<4>(filtered, raw, H, W, s);
    default: return unfilter_bands<6>(filtered, raw, H, W, s);
  }
}

extern "C" int pcfa_samples_to_planar(const unsigned char* raw, int H, int W, int kind, float* out, int Hp, int Wp,
                                      void* stream) {
  if (!raw || !out || H < 1 || W < 1 || Hp < 1 || Wp < 1 || kind < KIND_RGB8 || kind > KIND_KITTI_FLOW16 ||
      (reinterpret_cast<uintptr_t>(out) & 3) != 0)
    return PCFA_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  switch (kind) {
    case KIND_RGB8: planar_launch<KIND_RGB8, 3>(raw, H, W, out, Hp, Wp, s); break;
    case KIND_GREY8: planar_launch<KIND_GREY8, 1>(raw, H, W, out, Hp, Wp, s); break;
    case KIND_RGBA8: planar_launch<KIND_RGBA8, 4>(raw, H, W, out, Hp, Wp, s); break;
    default: planar_launch<KIND_KITTI_FLOW16, 6>(raw, H, W, out, Hp, Wp, s); break;
  }
  PCFA_LAUNCH_CHECK();
  return PCFA_OK;
}
