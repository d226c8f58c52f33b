// What the two batch zip readers share (zh_zip_open_batch.hip: openZipArchive of ziparchives.nim; zh_zip_read_batch.hip:
// ZipArchive.open of ziparchives_v1.nim): little-endian field loads, the bounds rule, the per-archive first-failure
// reduction, and the guards of a call's host buffers and readers.  The kernel has internal linkage: each file that
// includes this header launches its own copy.
#pragma once
#include "zh_host.h"
#include "zh_zip_reader.h"

namespace {

constexpr uint32_t kNone = 0xffffffffu;

// little-endian fields at any alignment
__device__ __forceinline__ uint32_t ld16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}
__device__ __forceinline__ uint64_t ld64(const uint8_t* p) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}
// [at, at + n) lies inside an image of `size` bytes (zh_zip.hip's Image::has: no additions on untrusted values)
__device__ __forceinline__ bool has(int64_t size, int64_t at, int64_t n) {
  return at >= 0 && n >= 0 && n <= size && at <= size - n;
}

// One workgroup per range: of the items [ranges[2r], ranges[2r + 1]) the first whose status is not ZH_OK (kNone if
// there is none) -- the serial loop stops there --, and whether any of them carries a flag.
__global__ __launch_bounds__(256) void zh_zip_reduce_kernel(const uint32_t* __restrict__ ranges,
                                                            const int32_t* __restrict__ st,
                                                            const uint8_t* __restrict__ flag,
                                                            uint32_t* __restrict__ first_bad,
                                                            uint32_t* __restrict__ any_flag) {
  __shared__ uint32_t wave_min[4], wave_any[4];
  const uint32_t lo = ranges[2 * blockIdx.x], hi = ranges[2 * blockIdx.x + 1];
  uint32_t best = kNone, any = 0;
  for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) {
    if (best == kNone && st[i] != ZH_OK) best = i;
    if (flag && flag[i]) any = 1;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    best = min(best, (uint32_t)__shfl_xor(best, m));
    any |= (uint32_t)__shfl_xor(any, m);
  }
  if (zh_lane() == 0) {
    wave_min[threadIdx.x >> 6] = best;
    wave_any[threadIdx.x >> 6] = any;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    first_bad[blockIdx.x] = min(min(wave_min[0], wave_min[1]), min(wave_min[2], wave_min[3]));
    any_flag[blockIdx.x] = wave_any[0] | wave_any[1] | wave_any[2] | wave_any[3];
  }
}

struct HostBufs {  // host buffers of the call that no reader owns yet
  std::vector<void*> p;
  ~HostBufs() {
    for (void* q : p) free(q);
  }
};
struct Readers {  // the readers of the call until it succeeds
  std::vector<zh_zip_reader*> r;
  ~Readers() {
    for (zh_zip_reader* q : r) zh_zip_close(q);
  }
};

uint64_t round_up8(uint64_t x) { return (x + 7) & ~(uint64_t)7; }

}  // namespace
