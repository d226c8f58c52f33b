// Byte ranges written to unaligned places with 16-byte stores -- the one copy of it: Chunk16, gather16 (sixteen bytes
// at any source alignment), write_range (a range whose bytes a generator makes) and copy_range (a range copied from a
// differently aligned source), a wave a range.  zh_zip_write.hip's writers, zh_zip_dev.h's finish kernel for the stored
// entries of both batch zip readers and zh_bgzf.hip's assemble kernel write their ranges through these; zh_ranges.hip's
// clip kernel, a workgroup a range, keeps a loop of its own over gather16; zh_scan.h's signature
// scan and zh_tar_create.hip's header kernel use Chunk16 alone.
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

template <class Gen>
__device__ __forceinline__ Chunk16 bytes16(const Gen& g, uint64_t c) {
  Chunk16 v{{0, 0, 0, 0}};
#pragma unroll
  for (uint32_t k = 0; k < 16; k++) v.w[k >> 2] |= g.byte(c + k) << (8 * (k & 3));
  return v;
}

// One wave writes the range [a, b) of out, a 16-byte aligned address: the bytes in front of the first and behind the
// last aligned 16-byte chunk one a lane, every whole chunk in between with one 16-byte store.  g.byte(q) is the byte
// at q; chunks at or past `copy_at` take their bytes straight from slots + copy_src + (chunk - copy_at).  Ranges of
// different waves never share a byte, so no byte is written twice.
template <class Gen>
__device__ __forceinline__ void write_range(uint8_t* __restrict__ out, uint64_t a, uint64_t b, uint32_t lane,
                                            const Gen& g, uint64_t copy_at = ~0ull,
                                            const uint8_t* __restrict__ slots = nullptr, uint64_t copy_src = 0) {
  if (a >= b) return;
  const uint64_t A = (a + 15) & ~(uint64_t)15, B = b & ~(uint64_t)15;
  if (A >= B) {  // no whole chunk inside: at most 30 bytes
    if (a + lane < b) out[a + lane] = (uint8_t)g.byte(a + lane);
    return;
  }
  if (a + lane < A) out[a + lane] = (uint8_t)g.byte(a + lane);
  if (B + lane < b) out[B + lane] = (uint8_t)g.byte(B + lane);
  for (uint64_t c = A + 16ull * lane; c < B; c += 1024) {
    const Chunk16 v = c >= copy_at ? gather16(slots, copy_src + (c - copy_at)) : bytes16(g, c);
    *reinterpret_cast<Chunk16*>(out + c) = v;
  }
}

// ... the plain copy: out[q] = in[q + delta] (mod 2^64) for q in [a, b), every whole chunk gathered.  `in` stays
// readable kGatherSlack bytes past its last source byte.
struct CopyGen {
  const uint8_t* __restrict__ in;
  uint64_t delta;
  __device__ uint32_t byte(uint64_t q) const { return in[q + delta]; }
};
__device__ __forceinline__ void copy_range(uint8_t* __restrict__ out, uint64_t a, uint64_t b,
                                           const uint8_t* __restrict__ in, uint64_t delta, uint32_t lane) {
  write_range(out, a, b, lane, CopyGen{in, delta}, 0, in, delta);
}

}  // namespace
