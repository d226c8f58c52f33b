// The signature scan that the walks over found candidates start with (zh_zip_read_batch.hip: the three zip
// signatures; zh_bgzf.hip: the first four bytes of a BGZF member): every 16-byte chunk of an upload is read once a
// pass (count, then write), and the positions whose four bytes satisfy the caller's predicate and lie inside ONE image
// are the hits, sorted by position.  Scratch: 8 bytes per hit, 4 per 16 KiB of the upload; nothing per image byte.
// The kernels have internal linkage: each file that includes this header launches its own copy.
// Below the kernels, the host half both files drive them with: the layout and upload of the images (scan_upload), the
// two passes, the read-back of the number of hits and the rounds of doubling they allow (scan_hits, templated on the
// predicate) and the walk's scratch with the caller's arrays behind it (scan_walk_alloc).  A format's own `ranges`,
// `next` and `parse` kernels, and everything behind the walk, are its file's.
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

// ---------------------------------------------------------------------------
// host: the upload, the two passes, and the walk's scratch sized by the hits
// ---------------------------------------------------------------------------
// A call's images on the device, and the hits of the scan over them (two owners: the hits are the walk's, the upload
// lives as long as anything is decoded from it).  The launches of the callers take d_in.p, imgs() and hits() as plain
// pointers of their own, never a DevBuf or one of these structs: a launch must not take the guard of a buffer along.
struct ScanUpload {
  DevBuf d_in, d_imgs;
  std::vector<uint64_t> up_off;  // where image t lies in d_in
  uint64_t up_total = 0;
  uint64_t max_chain = 0;  // the most records one image has room for
  uint32_t n_img = 0;
  const ZhZrImg* imgs() const { return reinterpret_cast<const ZhZrImg*>(d_imgs.p); }
};
struct ScanHits {
  DevBuf d_sums, d_hits;  // the groups' sums; the positions, ascending
  uint32_t n_hits = 0, rounds = 0;  // rounds: of doubling, for the longest chain there can be
  const uint64_t* hits() const { return reinterpret_cast<const uint64_t*>(d_hits.p); }
};

inline std::string scan_label(const char* what, const char* phase) { return std::string(what) + ": " + phase; }

// One upload: every image at an 8-byte aligned offset of ONE allocation that ends with 512 spare bytes (the plan reads
// whole aligned words around a source, the scan aligned 16-byte chunks), and the table of the images.  min_record: no
// record of the format is shorter.  ZH_ERR_ARGUMENT for more nodes or images than the walk's 32 bits count (two
// signatures do not overlap: at most one node every four bytes, and one an image).  n > 0.
inline int scan_upload(zh_ctx* ctx, Trace& tr, const char* what, const void* const* images, const size_t* lens,
                       size_t n, uint32_t min_record, ScanUpload& S) {
  std::vector<ZhZrImg> imgs(n);
  std::vector<uint64_t> up_len(n);
  S.up_off.assign(n, 0);
  uint64_t up_total = 0, most_nodes = 0;
  for (size_t t = 0; t < n; t++) {
    imgs[t] = ZhZrImg{up_total, (uint64_t)lens[t]};
    S.up_off[t] = up_total;
    up_len[t] = lens[t];
    up_total += ((uint64_t)lens[t] + 7) & ~(uint64_t)7;
    most_nodes += lens[t] / 4 + 1;
    S.max_chain = std::max<uint64_t>(S.max_chain, lens[t] / min_record + 1);
  }
  if (most_nodes >= 0xffffffffull || n >= 0x7fffffffull) return ZH_ERR_ARGUMENT;
  S.up_total = up_total;
  S.n_img = (uint32_t)n;
  ZH_HIP(ctx, hipSetDevice(ctx->device));
  int st;
  if (dev_alloc(ctx, S.d_in, up_total + 512) != hipSuccess) return ZH_ERR_NOMEM;
  if (up_total && (st = zhh_upload_slices(ctx, images, S.up_off, up_len, up_total, S.d_in.p))) return st;
  std::vector<uint64_t> ioff;
  if ((st = zhh_upload_spans(ctx, {{imgs.data(), n * sizeof(ZhZrImg)}}, S.d_imgs, ioff))) return st;
  tr.mark(ctx, scan_label(what, "upload").c_str());
  return ZH_OK;
}

// The scan over the upload, count pass and write pass: H.n_hits, H.hits(), H.rounds.  Under ZH_TRACE each pass is
// timed by itself between HIP events.
template <class Pred>
int scan_hits(zh_ctx* ctx, Trace& tr, const char* what, const ScanUpload& S, ScanHits& H) {
  hipStream_t s = ctx->stream;
  const dim3 wg(256);
  const uint8_t* const in = S.d_in.p;
  const ZhZrImg* const dimgs = S.imgs();
  const uint32_t n_img = S.n_img;
  const uint64_t scan_bytes = (S.up_total + 15) & ~(uint64_t)15;
  const uint64_t n_groups64 = std::max<uint64_t>(1, (scan_bytes + kScanGroupBytes - 1) / kScanGroupBytes);
  if (n_groups64 >= 0x7fffffffull) return ZH_ERR_ARGUMENT;
  const uint32_t n_groups = (uint32_t)n_groups64;
  if (dev_alloc(ctx, H.d_sums, ((size_t)n_groups + 1) * 4) != hipSuccess) return ZH_ERR_NOMEM;
  uint32_t* const gsums = reinterpret_cast<uint32_t*>(H.d_sums.p);
  Events evs;
  if (tr.on) evs.create();
  if (evs.ok) (void)hipEventRecord(evs.e[0], s);
  hipLaunchKernelGGL((zh_sig_scan_kernel<false, Pred>), dim3(n_groups), wg, 0, s, in, scan_bytes, dimgs, n_img, gsums,
                     (uint64_t*)nullptr);
  if (evs.ok) (void)hipEventRecord(evs.e[1], s);
  hipLaunchKernelGGL(zh_walk_scan_offsets_kernel, dim3(1), wg, 0, s, gsums, n_groups);
  ZH_HIP(ctx, hipGetLastError());
  uint32_t n_hits = 0;  // everything behind the scan is sized by the hits there are
  ZH_HIP(ctx, hipMemcpyAsync(&n_hits, gsums + n_groups, 4, hipMemcpyDeviceToHost, s));
  ZH_HIP(ctx, hipStreamSynchronize(s));
  H.n_hits = n_hits;
  if (dev_alloc(ctx, H.d_hits, (size_t)n_hits * 8 + 256) != hipSuccess) return ZH_ERR_NOMEM;
  uint64_t* const hits = reinterpret_cast<uint64_t*>(H.d_hits.p);
  if (evs.ok) (void)hipEventRecord(evs.e[2], s);
  if (n_hits)
    hipLaunchKernelGGL((zh_sig_scan_kernel<true, Pred>), dim3(n_groups), wg, 0, s, in, scan_bytes, dimgs, n_img, gsums, hits);
  if (evs.ok) {
    (void)hipEventRecord(evs.e[3], s);
    fprintf(stderr, "[zh] %-28s %8.3f ms (HIP events; count pass: %llu bytes read)\n",
            scan_label(what, "scan kernel 1").c_str(), evs.ms(0, 1), (unsigned long long)scan_bytes);
    fprintf(stderr, "[zh] %-28s %8.3f ms (HIP events; write pass: %u hits, at most %llu bytes read)\n",
            scan_label(what, "scan kernel 2").c_str(), evs.ms(2, 3), n_hits,
            (unsigned long long)std::min<uint64_t>(scan_bytes, (uint64_t)n_hits * kScanGroupBytes));
  }
  tr.mark(ctx, scan_label(what, "scan").c_str());
  // after `rounds` rounds of doubling every node up to 2^rounds - 1 steps from a start is marked; a chain has no more
  // records than there are hits, nor than its image has room for
  const uint64_t max_chain = std::min<uint64_t>(S.max_chain, n_hits);
  while ((1ull << H.rounds) < max_chain + 1) H.rounds++;
  return ZH_OK;
}

// The walk's scratch over the hits and one END node an image, and behind it the arrays the caller declared in `ex`
inline int scan_walk_alloc(zh_ctx* ctx, const ScanUpload& S, const ScanHits& H, Arena& ex, Walk& w) {
  if (const int st = walk_alloc(ctx, w, H.n_hits + S.n_img, ex.size + 256)) return st;
  ex.base = w.extra;
  ex.bind();
  return ZH_OK;
}

}  // namespace
