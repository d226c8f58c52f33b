// What the four batch readers' walks share (zh_tar_open_batch.hip, zh_tar_read_batch.hip, zh_zip_open_batch.hip,
// zh_zip_read_batch.hip): a chain of records whose positions are sums of the variable lengths before them is found in
// parallel.  Every candidate position ("node") gets next[b] as if a record started there; the nodes reachable from a
// start ARE the records:
//   zh_walk_double_kernel  pointer doubling with marks
//   zh_walk_scan_*         a prefix sum over the marks: every record's ordinal in walk order, the list of records
//   zh_walk_rec_ranges_kernel  every image's range of that list, for the walks over scanned candidates (zh_scan.h)
// and the host half that launches them (Walk).  What a node is, and next[b], is the caller's.
// The kernels have internal linkage: each file that includes this header launches its own copy.
#pragma once
#include "zh_host.h"

namespace {

constexpr uint32_t kScanItems = 1024;  // nodes a workgroup of the scan covers

// exclusive prefix sum of v over the 256 threads of the workgroup, *total = the sum
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* total) {
  __shared__ uint32_t wave_sum[4];
  const uint32_t incl = zh_wave_scan(v), wave = threadIdx.x >> 6;
  __syncthreads();  // (the previous call's reads of wave_sum are over)
  if (zh_lane() == 63) wave_sum[wave] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) {
    before += k < wave ? wave_sum[k] : 0u;
    all += wave_sum[k];
  }
  *total = all;
  return before + incl - v;
}

// One round of pointer doubling: every marked node marks the node its jump points to, then jump = jump o jump (from
// jin into jout).  Entering round r, jump is next^(2^r) and every node up to 2^r - 1 steps from a start is marked; a
// node marked early by a neighbour of the same round only marks other reachable nodes early.  END, the only fixed
// point, is never marked.  The marks are plain stores of the same value.
__global__ __launch_bounds__(256) void zh_walk_double_kernel(const uint32_t* __restrict__ jin,
                                                             uint32_t* __restrict__ jout, uint32_t* mark,
                                                             uint32_t n_nodes) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n_nodes) return;
  const uint32_t t = jin[b], tt = jin[t];
  if (mark[b] && tt != t) mark[t] = 1u;
  jout[b] = tt;
}

// The prefix sum over the marks, in three launches.  sums: marks per workgroup of kScanItems nodes.
__global__ __launch_bounds__(256) void zh_walk_scan_sums_kernel(const uint32_t* __restrict__ mark, uint32_t n_nodes,
                                                                uint32_t* __restrict__ sums) {
  const uint32_t base = blockIdx.x * kScanItems;
  uint32_t v = 0;
  for (uint32_t j = 0; j < kScanItems; j += 256) {
    const uint32_t b = base + j + threadIdx.x;
    v += b < n_nodes ? mark[b] : 0u;
  }
  uint32_t total;
  (void)block_scan(v, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// ... one workgroup turns them into the marks before each workgroup's nodes; sums[n_sums] = all marks (the records)
__global__ __launch_bounds__(256) void zh_walk_scan_offsets_kernel(uint32_t* sums, uint32_t n_sums) {
  uint32_t carry = 0;
  for (uint32_t j = 0; j < n_sums; j += 256) {
    const uint32_t i = j + threadIdx.x;
    const uint32_t v = i < n_sums ? sums[i] : 0u;
    uint32_t total;
    const uint32_t excl = block_scan(v, &total);
    if (i < n_sums) sums[i] = carry + excl;
    carry += total;
  }
  if (threadIdx.x == 0) sums[n_sums] = carry;
}
// ... ord[b] = marks before node b, in walk order across the whole call; list[ord[b]] = b for every record
__global__ __launch_bounds__(256) void zh_walk_scan_write_kernel(const uint32_t* __restrict__ mark, uint32_t n_nodes,
                                                                 const uint32_t* __restrict__ sums,
                                                                 uint32_t* __restrict__ ord,
                                                                 uint32_t* __restrict__ list) {
  const uint32_t base = blockIdx.x * kScanItems;
  uint32_t carry = sums[blockIdx.x];
  for (uint32_t j = 0; j < kScanItems; j += 256) {
    const uint32_t b = base + j + threadIdx.x;
    const uint32_t v = b < n_nodes ? mark[b] : 0u;
    uint32_t total;
    const uint32_t at = carry + block_scan(v, &total);
    if (b < n_nodes) {
      ord[b] = at;
      if (v) list[at] = b;
    }
    carry += total;
  }
}

// Where the nodes are found candidates in image order (zh_scan.h), ranges[2t .. 2t + 1] being image t's: image t's
// records are those between the ordinals of its first candidate and of the next image's (ord[all candidates] = all
// records)
__global__ __launch_bounds__(256) void zh_walk_rec_ranges_kernel(const uint32_t* __restrict__ ranges, uint32_t n_img,
                                                                 const uint32_t* __restrict__ ord,
                                                                 uint32_t* __restrict__ rec_ranges) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_img) return;
  rec_ranges[2 * t] = ord[ranges[2 * t]];
  rec_ranges[2 * t + 1] = ord[ranges[2 * t + 1]];
}

// The walk's scratch: two jump arrays, the marks, the ordinals -- 4 bytes a node each --, the scan's workgroup sums,
// and `extra` bytes of the caller's behind them.  The caller's `next` kernel fills j0 and mark.
struct Walk {
  DevBuf scr;
  uint32_t N = 0, n_sums = 0;
  uint32_t *j0 = nullptr, *j1 = nullptr, *mark = nullptr, *ord = nullptr, *sums = nullptr;
  uint32_t* list = nullptr;  // = j0: the jump arrays are dead behind the doubling, the list of records takes their place
  uint8_t* extra = nullptr;
};
inline int walk_alloc(zh_ctx* ctx, Walk& w, uint32_t n_nodes, size_t extra = 0) {
  const size_t N = w.N = n_nodes;
  w.n_sums = (n_nodes + kScanItems - 1) / kScanItems;
  Arena ar;
  ar.add(w.j0, N);
  ar.add(w.j1, N);
  ar.add(w.mark, N);
  ar.add(w.ord, N);
  ar.add(w.sums, (size_t)w.n_sums + 1);
  ar.add(w.extra, extra);
  if (ar.alloc(ctx, w.scr) != hipSuccess) return ZH_ERR_NOMEM;
  ar.bind();
  w.list = w.j0;
  return ZH_OK;
}
// `rounds` rounds of doubling on stream s: every node up to 2^rounds - 1 steps from a start is marked.
// (Plain pointers for the launches here and below: a launch must not take the Walk, that is its DevBuf, along.)
inline void walk_double(const Walk& w, uint32_t rounds, hipStream_t s) {
  const uint32_t N = w.N;
  uint32_t *jin = w.j0, *jout = w.j1, *const mark = w.mark;
  for (uint32_t r = 0; r < rounds; r++) {
    hipLaunchKernelGGL(zh_walk_double_kernel, dim3((N + 255) / 256), dim3(256), 0, s, (const uint32_t*)jin, jout, mark, N);
    std::swap(jin, jout);
  }
}
// ... then the scan over the marks: ord[] and list[]; nothing is waited for
inline void walk_scan(const Walk& w, hipStream_t s) {
  const uint32_t N = w.N, n_sums = w.n_sums;
  uint32_t *const mark = w.mark, *const sums = w.sums, *const ord = w.ord, *const list = w.list;
  const dim3 wg(256);
  hipLaunchKernelGGL(zh_walk_scan_sums_kernel, dim3(n_sums), wg, 0, s, (const uint32_t*)mark, N, sums);
  hipLaunchKernelGGL(zh_walk_scan_offsets_kernel, dim3(1), wg, 0, s, sums, n_sums);
  hipLaunchKernelGGL(zh_walk_scan_write_kernel, dim3(n_sums), wg, 0, s, (const uint32_t*)mark, N,
                     (const uint32_t*)sums, ord, list);
}
// ... and the number of records comes back (what follows is sized by them, not by the nodes): this waits
inline int walk_count(zh_ctx* ctx, const Walk& w, uint32_t* n_rec) {
  ZH_HIP(ctx, hipGetLastError());
  ZH_HIP(ctx, hipMemcpyAsync(n_rec, w.sums + w.n_sums, 4, hipMemcpyDeviceToHost, ctx->stream));
  ZH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ZH_OK;
}

}  // namespace
