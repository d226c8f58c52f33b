// The signature scan that the walks over found candidates start with (zh_zip_read_batch.hip: the three zip
// signatures; zh_bgzf.hip: the first four bytes of a BGZF member): every 16-byte chunk of an upload is read once a
// pass (count, then write), and the positions whose four bytes satisfy the caller's predicate and lie inside ONE image
// are the hits, sorted by position.  Scratch: 8 bytes per hit, 4 per 16 KiB of the upload; nothing per image byte.
// The kernels have internal linkage: each file that includes this header launches its own copy.
#pragma once
#include "zh_gather.h"
#include "zh_walk.h"

namespace {

// the scan: a lane reads 16 bytes, a wave 1024 contiguous bytes, a workgroup 4096 a step, kScanSteps steps
constexpr uint32_t kScanSteps = 4;
constexpr uint64_t kScanStepBytes = 256 * 16, kScanGroupBytes = kScanStepBytes * kScanSteps;

struct ZhZrImg {
  uint64_t up_off, len;  // where the image lies in the upload buffer
};

// the last image whose up_off <= p
__device__ __forceinline__ uint32_t find_img(const ZhZrImg* __restrict__ imgs, uint32_t n_img, uint64_t p) {
  uint32_t lo = 0, hi = n_img;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (imgs[mid].up_off <= p)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}
// the first of hits[lo, hi) that is >= p (hi if there is none)
__device__ __forceinline__ uint32_t lower_bound(const uint64_t* __restrict__ hits, uint32_t lo, uint32_t hi, uint64_t p) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (hits[mid] < p)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// The 16 positions of the chunk at `at` (a multiple of 16) as a mask of hits: x = the chunk's words, nw = the word
// behind it.  A candidate counts only inside one image.
template <class Pred>
__device__ __forceinline__ uint32_t chunk_hits(const Chunk16& x, uint32_t nw, uint64_t at,
                                               const ZhZrImg* __restrict__ imgs, uint32_t n_img) {
  const uint32_t w[5] = {x.w[0], x.w[1], x.w[2], x.w[3], nw};
  uint32_t m = 0;
#pragma unroll
  for (uint32_t j = 0; j < 16; j++)
    if (Pred::match(__builtin_amdgcn_alignbyte(w[(j >> 2) + 1], w[j >> 2], j & 3))) m |= 1u << j;
  for (uint32_t rest = m; rest; rest &= rest - 1) {  // (rare: a handful a record)
    const uint32_t j = (uint32_t)__ffs(rest) - 1;
    const ZhZrImg g = imgs[find_img(imgs, n_img, at + j)];
    if (at + j + 4 > g.up_off + g.len) m &= ~(1u << j);
  }
  return m;
}

// The signature scan over the upload's bytes [0, n_bytes), n_bytes a multiple of 16.  A workgroup covers
// kScanGroupBytes in kScanSteps steps; in a step a wave reads 1024 contiguous bytes, one aligned 16-byte load a lane.
// The three bytes behind a lane's chunk come from its neighbour's registers (lane 63: one more word, of a line the
// wave's next step reads anyway).  WRITE = false: sums[group] = the group's hits.  WRITE = true: sums[group] = the
// hits before the group (sums[groups] = all hits); the positions go to hits[] in ascending order, and only the groups
// that hold a hit read their bytes a second time.
template <bool WRITE, class Pred>
__global__ __launch_bounds__(256) void zh_sig_scan_kernel(const uint8_t* __restrict__ d_in, uint64_t n_bytes,
                                                          const ZhZrImg* __restrict__ imgs, uint32_t n_img,
                                                          uint32_t* __restrict__ sums, uint64_t* __restrict__ hits) {
  const uint64_t base = (uint64_t)blockIdx.x * kScanGroupBytes + 16ull * threadIdx.x;
  uint32_t carry = WRITE ? sums[blockIdx.x] : 0u, count = 0;
  if (WRITE && sums[blockIdx.x + 1] == carry) return;  // no hit in this group: its bytes are not read again
#pragma unroll
  for (uint32_t step = 0; step < kScanSteps; step++) {
    const uint64_t at = base + step * kScanStepBytes;
    const bool live = at < n_bytes;
    Chunk16 x{};
    if (live) x = *reinterpret_cast<const Chunk16*>(d_in + at);
    uint32_t nw = (uint32_t)__shfl_down(x.w[0], 1);
    if (live && zh_lane() == 63) nw = *reinterpret_cast<const uint32_t*>(d_in + at + 16);  // (the spare bytes at the latest)
    const uint32_t m = live ? chunk_hits<Pred>(x, nw, at, imgs, n_img) : 0u;
    if (!WRITE) {
      count += (uint32_t)__popc(m);
    } else {
      uint32_t total;
      uint32_t k = carry + block_scan((uint32_t)__popc(m), &total);
      for (uint32_t rest = m; rest; rest &= rest - 1) hits[k++] = at + (uint32_t)__ffs(rest) - 1;
      carry += total;
    }
  }
  if (!WRITE) {
    uint32_t total;
    (void)block_scan(count, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
  }
}

}  // namespace
