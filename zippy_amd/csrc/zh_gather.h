// Sixteen bytes at any source alignment, for kernels that copy byte ranges between unaligned places with 16-byte
// stores (zh_zip_write.hip's writers; zh_zip_dev.h's finish kernel for the stored entries of both batch zip readers;
// zh_zip_read_batch.hip's signature scan loads its chunks as Chunk16).
#pragma once
#include "zh_common.h"

namespace {

struct alignas(16) Chunk16 {
  uint32_t w[4];
};

// out word k = bytes [4 * (W0 + k) + b, + 4) of w: one alignbyte a word
template <int W0>
__device__ __forceinline__ Chunk16 funnel(const uint32_t (&w)[8], uint32_t b) {
  Chunk16 r;
#pragma unroll
  for (int k = 0; k < 4; k++) r.w[k] = __builtin_amdgcn_alignbyte(w[W0 + k + 1], w[W0 + k], b);
  return r;
}

constexpr uint64_t kGatherSlack = 31;  // gather16 reads at most this far past its last source byte

// Sixteen source bytes at s (any alignment) from two aligned 16-byte loads, recombined.  s & 15 is the same for every
// chunk of a range (source and destination advance together), so the branches are uniform across the wave.  The
// second load reads at most 31 bytes past s: the caller keeps that much readable behind its last source byte (an
// output slot's 256-byte rounding, a buffer's spare bytes).
__device__ __forceinline__ Chunk16 gather16(const uint8_t* __restrict__ base, uint64_t s) {
  const Chunk16* p = reinterpret_cast<const Chunk16*>(base + (s & ~(uint64_t)15));
  const uint32_t sh = (uint32_t)(s & 15);
  const Chunk16 x = p[0];
  if (sh == 0) return x;
  const Chunk16 y = p[1];
  const uint32_t w[8] = {x.w[0], x.w[1], x.w[2], x.w[3], y.w[0], y.w[1], y.w[2], y.w[3]};
  switch (sh >> 2) {
    case 0: return funnel<0>(w, sh & 3);
    case 1: return funnel<1>(w, sh & 3);
    case 2: return funnel<2>(w, sh & 3);
    default: return funnel<3>(w, sh & 3);
  }
}

}  // namespace
