// The arithmetic of pcfa_digest_words (include/pcfa_hip.h), stated once: the index mix h and the four terms one 32-bit
// word adds to a digest.  Host and device compile the same lines; tests/test_digest_gpu.py restates them in numpy.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PCFA_DIGEST_FN __host__ __device__ __forceinline__
#else
#define PCFA_DIGEST_FN static inline
#endif

// h(i): two multiply / xor-shift rounds over the 64-bit index, lowest bit forced to 1.  Odd, so that w * h(i) mod 2^64
// keeps every bit of w (an odd factor is invertible mod 2^64): a change of word i alone always changes the second sum.
PCFA_DIGEST_FN uint64_t pcfa_digest_h(uint64_t i) {
  uint64_t z = i * 0x9E3779B97F4A7C15ull;
  z ^= z >> 32;
  z *= 0xD6E8FEB86659FD93ull;
  z ^= z >> 32;
  return z | 1ull;
}

struct PcfaDigest {
  uint64_t sum, mixed, nan, inf;   // out4[0..3]
};

// adds word w with global index i
PCFA_DIGEST_FN void pcfa_digest_add(PcfaDigest& d, uint32_t w, uint64_t i) {
  const uint32_t mag = w & 0x7FFFFFFFu;
  d.sum += (uint64_t)w;
  d.mixed += (uint64_t)w * pcfa_digest_h(i);
  d.nan += mag > 0x7F800000u ? 1u : 0u;
  d.inf += mag == 0x7F800000u ? 1u : 0u;
}
