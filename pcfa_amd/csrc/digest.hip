// pcfa_digest_words: an exact, launch-independent bit digest of a buffer (include/pcfa_hip.h; arithmetic: digest.hpp).
//
// Workgroup b sums its share of the words in registers, reduces over the workgroup (shuffles, then 16 waves x 4 values of
// LDS) and stores its four partial sums at workspace[4 b]; a one-workgroup finish adds the partials into out4.  A buffer
// that one workgroup covers writes out4 directly (one launch).  Every sum is an integer sum mod 2^64, so neither the grid
// nor the order of anything changes a bit, and nothing has to be zeroed beforehand: no atomics, no memset node.
#include "common.hpp"
#include "digest.hpp"

namespace {

constexpr int DIGEST_THREADS = 1024;      // 16 waves; a thread keeps DIGEST_PIECES 16-byte loads in flight per trip
constexpr int DIGEST_MAX_BLOCKS = 256;    // one workgroup per CU; the grid-stride loop takes the rest
constexpr int DIGEST_PIECES = 3;
constexpr int DIGEST_FINISH_THREADS = 256;
static_assert(DIGEST_FINISH_THREADS >= DIGEST_MAX_BLOCKS, "the finish reads one partial per thread");

__device__ __forceinline__ uint64_t digest_wave_sum(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o);
  return v;
}

// dst[0..3] = the four sums of d over the workgroup (red: THREADS / 64 * 4 words of LDS)
template <int THREADS>
__device__ __forceinline__ void digest_block_store(const PcfaDigest& d, uint64_t* red, unsigned long long* dst) {
  const uint64_t s[4] = {digest_wave_sum(d.sum), digest_wave_sum(d.mixed), digest_wave_sum(d.nan), digest_wave_sum(d.inf)};
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) red[(threadIdx.x >> 6) * 4 + k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    uint64_t t = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) t += red[w * 4 + threadIdx.x];
    dst[threadIdx.x] = t;
  }
}

// x: n words; the first `head` (< 4) and the last n - head - 4 body4 (< 4) word by word in workgroup 0, the 16-byte
// aligned body between them as body4 pieces of four words, grid-stride.  A piece past the end is taken as four zero words:
// a zero word adds nothing to any of the four sums.
__global__ __launch_bounds__(DIGEST_THREADS) void digest_partial_kernel(const uint32_t* __restrict__ x,
                                                                        unsigned long long n,
                                                                        unsigned long long index0,
                                                                        unsigned long long head,
                                                                        unsigned long long body4,
                                                                        unsigned long long* __restrict__ dst) {
  __shared__ uint64_t red[DIGEST_THREADS / 64 * 4];
  PcfaDigest d{0, 0, 0, 0};
  const uint64_t stride = (uint64_t)gridDim.x * DIGEST_THREADS;
  const uint64_t gid = (uint64_t)blockIdx.x * DIGEST_THREADS + threadIdx.x;
  const uint4* body = reinterpret_cast<const uint4*>(x + head);
  const uint64_t base = index0 + head;
  for (uint64_t i = gid; i < body4; i += stride * DIGEST_PIECES) {
    uint4 v[DIGEST_PIECES];
#pragma unroll
    for (int k = 0; k < DIGEST_PIECES; ++k) {
      const uint64_t j = i + k * stride;
      v[k] = j < body4 ? body[j] : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int k = 0; k < DIGEST_PIECES; ++k) {
      const uint64_t g = base + 4 * (i + k * stride);
      pcfa_digest_add(d, v[k].x, g);
      pcfa_digest_add(d, v[k].y, g + 1);
      pcfa_digest_add(d, v[k].z, g + 2);
      pcfa_digest_add(d, v[k].w, g + 3);
    }
  }
  if (blockIdx.x == 0) {
    const uint64_t tail0 = head + 4 * body4, t = threadIdx.x;
    if (t < head) pcfa_digest_add(d, x[t], index0 + t);
    if (t >= 64 && tail0 + (t - 64) < n) pcfa_digest_add(d, x[tail0 + (t - 64)], index0 + tail0 + (t - 64));
  }
  digest_block_store<DIGEST_THREADS>(d, red, dst + 4 * (uint64_t)blockIdx.x);
}

__global__ __launch_bounds__(DIGEST_FINISH_THREADS) void digest_finish_kernel(const unsigned long long* __restrict__ part,
                                                                              int blocks,
                                                                              unsigned long long* __restrict__ out4) {
  __shared__ uint64_t red[DIGEST_FINISH_THREADS / 64 * 4];
  PcfaDigest d{0, 0, 0, 0};
  if ((int)threadIdx.x < blocks) {
    const unsigned long long* p = part + 4 * threadIdx.x;
    d = PcfaDigest{p[0], p[1], p[2], p[3]};
  }
  digest_block_store<DIGEST_FINISH_THREADS>(d, red, out4);
}

}  // namespace

extern "C" size_t pcfa_digest_workspace_bytes(void) { return (size_t)DIGEST_MAX_BLOCKS * 4 * sizeof(unsigned long long); }

extern "C" int pcfa_digest_words(const void* x, unsigned long long n_words, unsigned long long index0,
                                 unsigned long long* out4, void* workspace, void* stream) {
  const uintptr_t xa = reinterpret_cast<uintptr_t>(x);
  if ((!x && n_words != 0) || (xa & 3) != 0 || !out4 || (reinterpret_cast<uintptr_t>(out4) & 7) != 0 || !workspace ||
      (reinterpret_cast<uintptr_t>(workspace) & 7) != 0)
    return PCFA_ERR_INVALID_ARG;
  unsigned long long head = ((16 - (xa & 15)) & 15) >> 2;   // words in front of the first 16-byte boundary
  if (head > n_words) head = n_words;
  const unsigned long long body4 = (n_words - head) >> 2;
  unsigned long long blocks = (body4 + DIGEST_THREADS - 1) / DIGEST_THREADS;
  if (blocks < 1) blocks = 1;
  if (blocks > DIGEST_MAX_BLOCKS) blocks = DIGEST_MAX_BLOCKS;
  unsigned long long* part = blocks == 1 ? out4 : static_cast<unsigned long long*>(workspace);
  pcfa_launch(digest_partial_kernel, dim3((unsigned)blocks), dim3(DIGEST_THREADS), 0, (hipStream_t)stream,
              static_cast<const uint32_t*>(x), n_words, index0, head, body4, part);
  PCFA_LAUNCH_CHECK();
  if (blocks > 1) {
    pcfa_launch(digest_finish_kernel, dim3(1), dim3(DIGEST_FINISH_THREADS), 0, (hipStream_t)stream,
                static_cast<const unsigned long long*>(part), (int)blocks, out4);
    PCFA_LAUNCH_CHECK();
  }
  return PCFA_OK;
}
