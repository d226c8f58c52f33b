// BGZF, the blocked gzip of the SAM specification (section 4.1; bgzip, htslib): a file is a series of gzip members of
// at most 64 KiB, each with its total size in a `BC` extra subfield and its CRC-32 and ISIZE in its trailer, closed by
// an empty 28-byte member.  Every member is a raw-deflate stream of its own with its own checksum -- the batch shape
// of the engine --, and the index of a file is recovered from its headers and trailers without decoding anything.
//
// Writing (zh_bgzf_write_batch):
//   (plan)                    ONE compress plan over every piece of the call, CRC-32 requested; a piece whose stream
//                             outgrew ZH_BGZF_MAX_CDATA goes through a second, small plan at level 0 (5 + n bytes)
//   zh_bgzf_sizes_kernel      a member's size from its stream's length on the device
//   zh_bgzf_scan64_kernel     the prefix sum: a member's place
//   zh_bgzf_assemble_kernel   every byte of every image: headers, trailers and markers one byte a lane, CDATA from its
//                             slot to its place with aligned 16-byte stores (gather16), byte stores at the ragged ends
// Walking (zh_bgzf_read_batch, zh_bgzf_index_batch):
//   zh_sig_scan_kernel        the positions that hold 1f 8b 08 04 inside one image (zh_scan.h)
//   zh_bgzf_ranges_kernel     per image: its hits; what stands at byte 0 when that is no hit
//   zh_bgzf_next_kernel       where the member at a hit ends, that position found among the hits
//   zh_walk_double / scan     the hits reachable from byte 0 ARE the members (zh_walk.h)
//   zh_bgzf_parse_kernel      one fixed record a member; zh_bgzf_uoff_kernel: its place in the uncompressed data
// Reading: ONE raw-deflate uncompress plan over every member of the call, sources in place, CRC-32 requested;
//   zh_bgzf_verify_kernel     decoder status, then CRC-32 against the trailer, then length against ISIZE
//   zh_zip_reduce_kernel      per image (per range): the first member that failed, in file order
// Range reads (zh_bgzf_read_ranges): only the members a range touches go over the link; their headers are parsed
// again (zh_bgzf_parse_at_kernel), members wholly inside a range decode into its slot, the one or two at its ends
// into scratch and through zh_launch_range_clip.
// Shared host code: the upload of the images, the two passes of the scan and the walk's scratch are zh_scan.h's
// (scan_upload, scan_hits, scan_walk_alloc; zh_zip_read_batch.hip drives the same); pread's arithmetic, the merged
// spans of a range read's upload, the cut of a clip and the tail that hands results out are zh_range_host.h's
// (zh_ranges.hip uses the same).  What is BGZF's own stays here: member_at and the kernels built on it, the index's
// soundness, the members' slots.
// The host parses no header byte, compares no checksum and writes no byte of an image.
#include "zh_range_host.h"
#include "zh_scan.h"
#include "zh_zip_dev.h"

namespace {

constexpr uint32_t kBgzfMagic = 0x04088b1fu;  // 1f 8b 08 04
constexpr uint32_t kTaskBytes = 4096;         // CDATA bytes a wave of the assemble kernel moves

struct BgzfSignature {  // the scan's predicate (zh_scan.h)
  static __device__ __forceinline__ bool match(uint32_t v) { return v == kBgzfMagic; }
};

// What stands at a position if a member starts there: the checks in their order, the first that failed.
struct ZhBgzfHead {
  uint64_t end;  // the position behind the member
  uint32_t cdata_off, cdata_len, isize, crc;  // cdata_off: from the member's first byte
  int32_t status;
  uint32_t is_eof;  // byte for byte the 28-byte marker
};
// One reached member, for the host
struct ZhBgzfRec {
  uint64_t coff, cdata_off, uoff;  // coff, cdata_off: in the image; uoff: in the image's uncompressed data
  uint32_t cdata_len, isize, crc;
  int32_t status, succ_status;  // its own checks; what the walk finds where the next member should start
  uint32_t is_eof;
};

// a member at position pos of an image of len bytes (pos <= len)
__device__ __forceinline__ ZhBgzfHead member_at(const uint8_t* __restrict__ p, uint64_t len, uint64_t pos) {
  ZhBgzfHead h{};
  const uint64_t left = len - pos;
  const uint8_t* __restrict__ q = p + pos;
  auto fail = [&](int32_t st) {
    h.status = st;
    return h;
  };
  if (left < 12) return fail(ZH_ERR_INVALID_BUFFER);
  if (q[0] != 0x1f || q[1] != 0x8b) return fail(ZH_ERR_GZIP_ID);
  if (q[2] != 8) return fail(ZH_ERR_UNSUPPORTED_METHOD);
  const uint32_t flg = q[3];
  if (flg & 0xe0u) return fail(ZH_ERR_RESERVED_FLAGS);
  if (flg != 4) return fail(ZH_ERR_UNSUPPORTED_FLAGS);
  const uint32_t xlen = ld16(q + 10);
  if (12ull + xlen > left) return fail(ZH_ERR_INVALID_BUFFER);
  // the subfields (SI1, SI2, SLEN, data) tile XLEN; the first BC of two bytes says BSIZE
  uint32_t o = 0, bsize = kNone;
  bool tiled = true;
  while (o < xlen) {
    if (o + 4 > xlen) {
      tiled = false;
      break;
    }
    const uint8_t* __restrict__ f = q + 12 + o;
    const uint32_t slen = ld16(f + 2);
    if (o + 4 + slen > xlen) {
      tiled = false;
      break;
    }
    if (bsize == kNone && f[0] == 0x42 && f[1] == 0x43 && slen == 2) bsize = ld16(f + 4);
    o += 4 + slen;
  }
  if (!tiled || bsize == kNone) return fail(ZH_ERR_BGZF_HEADER);
  const uint32_t total = bsize + 1;
  if (total < 12 + xlen + 8) return fail(ZH_ERR_BGZF_HEADER);
  if (total > left) return fail(ZH_ERR_INVALID_BUFFER);
  h.end = pos + total;
  h.cdata_off = 12 + xlen;
  h.cdata_len = total - 8 - h.cdata_off;
  h.crc = ld32(q + total - 8);
  h.isize = ld32(q + total - 4);
  if (h.isize > 65536u) return fail(ZH_ERR_BGZF_HEADER);
  h.is_eof = total == 28 && ld32(q + 4) == 0 && ld32(q + 8) == 0x0006ff00u && ld32(q + 12) == 0x00024342u &&
             ld32(q + 16) == 0x0003001bu && ld32(q + 20) == 0 && ld32(q + 24) == 0;
  return h;
}

}  // namespace

// ---------------------------------------------------------------------------
// the walk
// ---------------------------------------------------------------------------
// Per image: ranges[2t .. 2t + 1] = its hits; start[t] = ZH_OK when its byte 0 is a hit or it is empty, else what
// the checks say of byte 0
__global__ __launch_bounds__(256) void zh_bgzf_ranges_kernel(const uint8_t* __restrict__ d_in,
                                                             const ZhZrImg* __restrict__ imgs, uint32_t n_img,
                                                             const uint64_t* __restrict__ hits, uint32_t n_hits,
                                                             uint32_t* __restrict__ ranges, int32_t* __restrict__ start) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_img) return;
  const ZhZrImg g = imgs[t];
  const uint32_t lo = lower_bound(hits, 0, n_hits, g.up_off), hi = lower_bound(hits, lo, n_hits, g.up_off + g.len);
  ranges[2 * t] = lo;
  ranges[2 * t + 1] = hi;
  int32_t st = ZH_OK;
  if (g.len && !(lo < hi && hits[lo] == g.up_off)) {
    st = member_at(d_in + g.up_off, g.len, 0).status;
    if (st == ZH_OK) st = ZH_ERR_INVALID_BUFFER;  // (cannot be: such a position is a hit)
  }
  start[t] = st;
}

// next[b] for every node b: nodes [0, n_hits) are the hits, node n_hits + t is image t's END (its own successor).  A
// hit's successor is the hit where its member ends; it is END when the member fails a check of its own, when it ends
// where the image ends, and when that position is no hit -- succ[b] then holds what the checks say there.
// mark[b] = 1 for byte 0 of an image.
__global__ __launch_bounds__(256) void zh_bgzf_next_kernel(const uint8_t* __restrict__ d_in,
                                                           const ZhZrImg* __restrict__ imgs, uint32_t n_img,
                                                           const uint64_t* __restrict__ hits, uint32_t n_hits,
                                                           const uint32_t* __restrict__ ranges, uint32_t n_nodes,
                                                           uint32_t* __restrict__ jump, uint32_t* __restrict__ mark,
                                                           int32_t* __restrict__ succ) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n_nodes) return;
  uint32_t nx = b, mk = 0;
  if (b < n_hits) {
    const uint64_t at = hits[b];
    const uint32_t t = find_img(imgs, n_img, at);
    const ZhZrImg g = imgs[t];
    const uint64_t pos = at - g.up_off;
    const ZhBgzfHead h = member_at(d_in + g.up_off, g.len, pos);
    int32_t sc = ZH_OK;
    nx = n_hits + t;
    if (h.status == ZH_OK && h.end != g.len) {
      const uint32_t hi = ranges[2 * t + 1], k = lower_bound(hits, b + 1, hi, g.up_off + h.end);
      if (k < hi && hits[k] == g.up_off + h.end) {
        nx = k;
      } else {
        sc = member_at(d_in + g.up_off, g.len, h.end).status;
        if (sc == ZH_OK) sc = ZH_ERR_INVALID_BUFFER;  // (cannot be: such a position is a hit)
      }
    }
    succ[b] = sc;
    mk = pos == 0 ? 1u : 0u;
  }
  jump[b] = nx;
  mark[b] = mk;
}

// One thread per reached member, in walk order (r = its ordinal in the call, list[r] its node); isz[r] = the bytes
// it promises (0 when its header failed)
__global__ __launch_bounds__(256) void zh_bgzf_parse_kernel(const uint8_t* __restrict__ d_in,
                                                            const ZhZrImg* __restrict__ imgs, uint32_t n_img,
                                                            const uint64_t* __restrict__ hits,
                                                            const uint32_t* __restrict__ list,
                                                            const int32_t* __restrict__ succ, uint32_t n_rec,
                                                            ZhBgzfRec* __restrict__ recs, uint32_t* __restrict__ isz) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rec) return;
  const uint32_t node = list[r];
  const uint64_t at = hits[node];
  const ZhZrImg g = imgs[find_img(imgs, n_img, at)];
  const uint64_t pos = at - g.up_off;
  const ZhBgzfHead h = member_at(d_in + g.up_off, g.len, pos);
  ZhBgzfRec rec{};
  rec.coff = pos;
  rec.cdata_off = pos + h.cdata_off;
  rec.cdata_len = h.cdata_len;
  rec.isize = h.isize;
  rec.crc = h.crc;
  rec.status = h.status;
  rec.succ_status = succ[node];
  rec.is_eof = h.is_eof;
  recs[r] = rec;
  isz[r] = h.status == ZH_OK ? h.isize : 0u;
}

// The members a range read touches, parsed where the index says they are: member m is the bytes [at[m], + avail[m])
// of the upload; it must end where they end and promise want[m] bytes, else ZH_ERR_INVALID_BUFFER.
__global__ __launch_bounds__(256) void zh_bgzf_parse_at_kernel(const uint8_t* __restrict__ d_in,
                                                               const uint64_t* __restrict__ at,
                                                               const uint32_t* __restrict__ avail,
                                                               const uint32_t* __restrict__ want, uint32_t n_mem,
                                                               ZhBgzfRec* __restrict__ recs) {
  const uint32_t m = blockIdx.x * 256 + threadIdx.x;
  if (m >= n_mem) return;
  const ZhBgzfHead h = member_at(d_in + at[m], avail[m], 0);
  ZhBgzfRec rec{};
  rec.coff = at[m];
  rec.cdata_off = at[m] + h.cdata_off;
  rec.cdata_len = h.cdata_len;
  rec.isize = h.isize;
  rec.crc = h.crc;
  rec.status = h.status;
  if (h.status == ZH_OK && (h.end != avail[m] || h.isize != want[m])) rec.status = ZH_ERR_INVALID_BUFFER;
  rec.is_eof = h.is_eof;
  recs[m] = rec;
}

// out[i] = v[0] + .. + v[i - 1] for i in [0, n]: one workgroup, 256 values a step (the values are sizes of members:
// a step's sum fits 32 bits)
__global__ __launch_bounds__(256) void zh_bgzf_scan64_kernel(const uint32_t* __restrict__ v, uint32_t n,
                                                             uint64_t* __restrict__ out) {
  uint64_t carry = 0;
  for (uint32_t j = 0; j < n; j += 256) {
    const uint32_t i = j + threadIdx.x;
    const uint32_t x = i < n ? v[i] : 0u;
    uint32_t total;
    const uint32_t excl = block_scan(x, &total);
    if (i < n) out[i] = carry + excl;
    carry += total;
  }
  if (threadIdx.x == 0) out[n] = carry;
}

// a member's place in the uncompressed data of its image, from the sums over the call
__global__ __launch_bounds__(256) void zh_bgzf_uoff_kernel(const ZhZrImg* __restrict__ imgs, uint32_t n_img,
                                                           const uint32_t* __restrict__ rec_ranges,
                                                           const uint64_t* __restrict__ sums, uint32_t n_rec,
                                                           ZhBgzfRec* __restrict__ recs) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rec) return;
  uint32_t lo = 0, hi = n_img;  // the last image whose records start at or before r and that has one
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (rec_ranges[2 * mid] <= r)
      lo = mid;
    else
      hi = mid;
  }
  recs[r].uoff = sums[r] - sums[rec_ranges[2 * lo]];
}

// Every member's verdict, by the first of these that applies: its header's status; the decoder's (out of room reads
// ZH_ERR_SIZE: more bytes than ISIZE promises); the CRC-32 against the trailer's; the length against ISIZE; what the
// walk found behind it.  pidx[r]: its stream in the plan.
__global__ __launch_bounds__(256) void zh_bgzf_verify_kernel(const ZhBgzfRec* __restrict__ recs,
                                                             const uint32_t* __restrict__ pidx, uint32_t n_rec,
                                                             const int32_t* __restrict__ plan_st,
                                                             const uint64_t* __restrict__ plan_len,
                                                             const uint32_t* __restrict__ plan_crc,
                                                             int32_t* __restrict__ est) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rec) return;
  const ZhBgzfRec e = recs[r];
  int32_t st = e.status;
  if (st == ZH_OK && pidx[r] != kNone) {
    const uint32_t k = pidx[r];
    st = plan_st[k];
    if (st == ZH_ERR_DST_TOO_SMALL)
      st = ZH_ERR_SIZE;
    else if (st == ZH_OK && plan_crc[k] != e.crc)
      st = ZH_ERR_CHECKSUM;
    else if (st == ZH_OK && plan_len[k] != e.isize)
      st = ZH_ERR_SIZE;
  }
  if (st == ZH_OK) st = e.succ_status;
  est[r] = st;
}

// ---------------------------------------------------------------------------
// the writer's kernels
// ---------------------------------------------------------------------------
namespace {

struct ZhBgzfMember {
  uint64_t slot;    // its stream in the slots of its plan
  uint64_t base;    // where its image starts in the output
  uint32_t first;   // the first member of its image
  uint32_t idx;     // its stream in its plan
  uint32_t cap;     // ... and that slot's size
  uint32_t usize;
  uint32_t which;   // 0: the call's plan, 1: the level-0 plan, 2: the EOF marker
  uint32_t pad;
};
struct ZhBgzfTask {
  uint32_t member, lo;  // CDATA bytes [lo, lo + kTaskBytes) of the member; lo == 0 also writes header and trailer
};

__device__ __forceinline__ uint32_t member_clen(const ZhBgzfMember& m, const uint64_t* __restrict__ len0,
                                                const uint64_t* __restrict__ len1) {
  const uint64_t n = m.which == 0 ? len0[m.idx] : len1[m.idx];
  return n < m.cap ? (uint32_t)n : m.cap;  // (a stream that failed says anything: its image is not handed out)
}

}  // namespace

__global__ __launch_bounds__(256) void zh_bgzf_sizes_kernel(const ZhBgzfMember* __restrict__ mem, uint32_t n_mem,
                                                            const uint64_t* __restrict__ len0,
                                                            const uint64_t* __restrict__ len1,
                                                            uint32_t* __restrict__ msize) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_mem) return;
  const ZhBgzfMember m = mem[k];
  msize[k] = m.which == 2 ? 28u : 26u + member_clen(m, len0, len1);
}

// every image's length: the sizes of its members
__global__ __launch_bounds__(256) void zh_bgzf_image_len_kernel(const uint32_t* __restrict__ mfirst, uint32_t n_img,
                                                                const uint64_t* __restrict__ mpos,
                                                                uint64_t* __restrict__ img_len) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t < n_img) img_len[t] = mpos[mfirst[t + 1]] - mpos[mfirst[t]];
}

// One wave per task (four a workgroup).  A member's first task writes its 18-byte header and its trailer (or the
// marker) one byte a lane; every task moves its piece of the CDATA from the slot to its (differently aligned) place
// by zh_gather.h's copy_range.
__global__ __launch_bounds__(256) void zh_bgzf_assemble_kernel(const uint8_t* __restrict__ slots0,
                                                               const uint8_t* __restrict__ slots1,
                                                               uint8_t* __restrict__ d_out,
                                                               const ZhBgzfMember* __restrict__ mem,
                                                               const ZhBgzfTask* __restrict__ tasks, uint32_t n_tasks,
                                                               const uint64_t* __restrict__ mpos,
                                                               const uint64_t* __restrict__ len0,
                                                               const uint64_t* __restrict__ len1,
                                                               const uint32_t* __restrict__ crc0,
                                                               const uint32_t* __restrict__ crc1) {
  const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = zh_lane();
  if (w >= n_tasks) return;
  const ZhBgzfTask t = tasks[w];
  const ZhBgzfMember m = mem[t.member];
  const uint64_t at = m.base + (mpos[t.member] - mpos[m.first]);
  if (m.which == 2) {
    const uint32_t marker[7] = {kBgzfMagic, 0u, 0x0006ff00u, 0x00024342u, 0x0003001bu, 0u, 0u};
    if (lane < 28) d_out[at + lane] = (uint8_t)(marker[lane >> 2] >> (8u * (lane & 3u)));
    return;
  }
  const uint32_t clen = member_clen(m, len0, len1);
  if (t.lo == 0) {
    const uint32_t bsize = 26u + clen - 1u;
    const uint32_t head[5] = {kBgzfMagic, 0u, 0x0006ff00u, 0x00024342u, bsize & 0xffffu};
    const uint32_t tail[2] = {m.which == 0 ? crc0[m.idx] : crc1[m.idx], m.usize};
    if (lane < 18) d_out[at + lane] = (uint8_t)(head[lane >> 2] >> (8u * (lane & 3u)));
    if (lane >= 32 && lane < 40) {
      const uint32_t j = lane - 32;
      d_out[at + 18 + clen + j] = (uint8_t)(tail[j >> 2] >> (8u * (j & 3u)));
    }
  }
  if (t.lo >= clen) return;
  const uint8_t* __restrict__ src = m.which == 0 ? slots0 : slots1;
  const uint64_t a = at + 18 + t.lo, b = at + 18 + (clen < t.lo + kTaskBytes ? clen : t.lo + kTaskBytes);
  copy_range(d_out, a, b, src, m.slot - (at + 18), lane);  // (slot byte = output byte + delta)
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
namespace {

// the bytes [from, to) of an arena back on the host in one copy (waits): h is an image of the arena's first `to`
// bytes in which Arena::host finds the arrays that lie in that stretch
int fetch(zh_ctx* ctx, std::vector<uint8_t>& h, const Arena& ar, size_t from, size_t to) {
  h.resize(to);
  if (to <= from) return ZH_OK;
  ZH_HIP(ctx, hipMemcpyAsync(h.data() + from, ar.base + from, to - from, hipMemcpyDeviceToHost, ctx->stream));
  ZH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ZH_OK;
}

// What the walk over a call's images leaves: the upload, and per image its records in file order.
struct BgzfWalk {
  ScanUpload S;  // (zh_scan.h)
  DevBuf d_rec;
  ZhBgzfRec* d_recs = nullptr;
  uint32_t* d_rec_ranges = nullptr;  // [2 * n_img]
  uint32_t n_rec = 0;
  std::vector<uint8_t> host;  // the download: what the three pointers below point into
  const ZhBgzfRec* recs = nullptr;
  const uint32_t* rec_ranges = nullptr;
  const int32_t* start = nullptr;  // what stands at byte 0 of an image whose walk never began
  // the walk of image t alone: its status, whether its last member is the marker
  int32_t walk_status(size_t t) const {
    if (start[t] != ZH_OK) return start[t];
    for (uint32_t r = rec_ranges[2 * t]; r < rec_ranges[2 * t + 1]; r++) {
      if (recs[r].status != ZH_OK) return recs[r].status;
      if (recs[r].succ_status != ZH_OK) return recs[r].succ_status;
    }
    return ZH_OK;
  }
  uint8_t has_eof(size_t t) const {
    const uint32_t lo = rec_ranges[2 * t], hi = rec_ranges[2 * t + 1];
    return walk_status(t) == ZH_OK && hi > lo && recs[hi - 1].is_eof ? 1 : 0;
  }
};

// The upload and the scan (zh_scan.h), the walk, the records.  n > 0.
int bgzf_walk(zh_ctx* ctx, Trace& tr, const void* const* images, const size_t* lens, size_t n, BgzfWalk& W) {
  int st;
  ScanUpload& S = W.S;
  ScanHits H;
  if ((st = scan_upload(ctx, tr, "bgzf", images, lens, n, 26, S))) return st;  // (no member is shorter than 26 bytes)
  if ((st = scan_hits<BgzfSignature>(ctx, tr, "bgzf", S, H))) return st;
  hipStream_t s = ctx->stream;
  const dim3 wg(256);
  const uint32_t n_img = S.n_img, n_hits = H.n_hits;
  const uint8_t* const in = S.d_in.p;
  const ZhZrImg* const dimgs = S.imgs();
  const uint64_t* const hits = H.hits();

  // the walk
  const uint32_t rounds = H.rounds, N = n_hits + n_img;
  int32_t *succ, *start;
  uint32_t* hit_ranges;
  Arena ex;
  ex.add(succ, n_hits);
  ex.add(hit_ranges, (size_t)n_img * 2);
  ex.add(start, n_img);
  Walk w;
  if ((st = scan_walk_alloc(ctx, S, H, ex, w))) return st;
  uint32_t *const j0 = w.j0, *const mark = w.mark;
  const uint32_t *const ord = w.ord, *const list = w.list;
  const dim3 node_grid((N + 255) / 256), img_grid((n_img + 255) / 256);
  hipLaunchKernelGGL(zh_bgzf_ranges_kernel, img_grid, wg, 0, s, in, dimgs, n_img, hits, n_hits,
                     hit_ranges, start);
  hipLaunchKernelGGL(zh_bgzf_next_kernel, node_grid, wg, 0, s, in, dimgs, n_img, hits, n_hits,
                     (const uint32_t*)hit_ranges, N, j0, mark, succ);
  walk_double(w, rounds, s);
  walk_scan(w, s);
  uint32_t n_rec = 0;
  if ((st = walk_count(ctx, w, &n_rec))) return st;
  W.n_rec = n_rec;
  tr.mark(ctx, "bgzf: reach + scan");

  // the records
  uint32_t* d_isz;
  uint64_t* d_usum;
  int32_t* d_start;
  Arena out;
  out.add(W.d_recs, n_rec);
  out.add(W.d_rec_ranges, (size_t)n_img * 2);
  out.add(d_start, n_img);
  const size_t out_bytes = out.size;  // (what comes back: the arrays so far, in one copy)
  out.add(d_isz, n_rec);
  out.add(d_usum, (size_t)n_rec + 1);
  if (out.alloc(ctx, W.d_rec, 256) != hipSuccess) return ZH_ERR_NOMEM;
  out.bind();
  ZhBgzfRec* const d_recs = W.d_recs;
  uint32_t* const d_rr = W.d_rec_ranges;
  const dim3 rec_grid((n_rec + 255) / 256);
  if (n_rec)
    hipLaunchKernelGGL(zh_bgzf_parse_kernel, rec_grid, wg, 0, s, in, dimgs, n_img, hits, list,
                       (const int32_t*)succ, n_rec, d_recs, d_isz);
  hipLaunchKernelGGL(zh_walk_rec_ranges_kernel, img_grid, wg, 0, s, (const uint32_t*)hit_ranges, n_img, ord, d_rr);
  hipLaunchKernelGGL(zh_bgzf_scan64_kernel, dim3(1), wg, 0, s, (const uint32_t*)d_isz, n_rec, d_usum);
  if (n_rec)
    hipLaunchKernelGGL(zh_bgzf_uoff_kernel, rec_grid, wg, 0, s, dimgs, n_img, (const uint32_t*)d_rr,
                       (const uint64_t*)d_usum, n_rec, d_recs);
  ZH_HIP(ctx, hipGetLastError());
  ZH_HIP(ctx, hipMemcpyAsync(d_start, start, (size_t)n_img * 4, hipMemcpyDeviceToDevice, s));
  if ((st = fetch(ctx, W.host, out, 0, out_bytes))) return st;
  W.recs = out.host(W.host.data(), (const ZhBgzfRec*)d_recs);
  W.rec_ranges = out.host(W.host.data(), (const uint32_t*)d_rr);
  W.start = out.host(W.host.data(), (const int32_t*)d_start);
  tr.mark(ctx, "bgzf: parse");
  return ZH_OK;
}

int images_there(const void* const* images, const size_t* lens, size_t n) {
  for (size_t t = 0; t < n; t++)
    if (!images[t] && lens[t]) return ZH_ERR_ARGUMENT;
  return ZH_OK;
}

// One raw-deflate plan over the members `planned` of d_recs (sources at src_off / src_len of `in`, slots at doff /
// dcap of `out`), CRC-32 requested; then every member's verdict in d_est
int decode_and_verify(zh_ctx* ctx, const uint8_t* in, uint8_t* out, const std::vector<uint64_t>& soff,
                      const std::vector<uint64_t>& slen, const std::vector<uint64_t>& doff,
                      const std::vector<uint64_t>& dcap, const ZhBgzfRec* d_recs, const uint32_t* d_pidx,
                      uint32_t n_rec, int32_t* d_est, PlanGuard& pg) {
  int st;
  const size_t n_plan = soff.size();
  if (n_plan) {
    if ((st = zh_plan_uncompress(ctx, n_plan, soff.data(), slen.data(), doff.data(), dcap.data(), ZH_DF_DEFLATE, &pg.p)) ||
        (st = zh_plan_request_crc32(pg.p, 1)) || (st = zh_plan_run(pg.p, in, out)))
      return st;
  }
  const int32_t* const plan_st = n_plan ? zh_plan_device_statuses(pg.p) : nullptr;
  const uint64_t* const plan_len = n_plan ? zh_plan_device_lens(pg.p) : nullptr;
  const uint32_t* const plan_crc = n_plan ? pg.p->buf_crc : nullptr;
  if (n_rec)
    hipLaunchKernelGGL(zh_bgzf_verify_kernel, dim3((n_rec + 255) / 256), dim3(256), 0, ctx->stream, d_recs, d_pidx,
                       n_rec, plan_st, plan_len, plan_crc, d_est);
  ZH_HIP(ctx, hipGetLastError());
  return ZH_OK;
}

}  // namespace

extern "C" int zh_bgzf_write_batch(zh_ctx* ctx, const void* const* srcs, const size_t* lens, size_t n, int level,
                                   size_t block_bytes, void** dsts, size_t* dst_lens, int32_t* statuses) {
  if (!ctx || (n && (!srcs || !lens || !dsts || !dst_lens || !statuses))) return ZH_ERR_ARGUMENT;
  clear_outputs(dsts, dst_lens, statuses, n);
  if (block_bytes > ZH_BGZF_MAX_BLOCK) return ZH_ERR_ARGUMENT;
  if (level < -2 || level > 9) {
    for (size_t i = 0; i < n; i++) statuses[i] = ZH_ERR_INVALID_LEVEL;
    return ZH_ERR_INVALID_LEVEL;
  }
  if (const int e = images_there(srcs, lens, n)) return e;
  if (!n) return ZH_OK;
  const uint64_t bb = block_bytes ? block_bytes : ZH_BGZF_BLOCK;
  ZH_HIP(ctx, hipSetDevice(ctx->device));
  Trace tr;
  int st;
  hipStream_t s = ctx->stream;
  const dim3 wg(256);

  // ---- 1. the sources go up; the pieces, their slots, the members and their tasks ----
  DevBuf d_src;
  std::vector<uint64_t> soff, slen;
  if ((st = zhh_upload(ctx, srcs, lens, n, d_src, soff, slen))) return st;
  tr.mark(ctx, "bgzf write: upload");
  std::vector<uint64_t> p_soff, p_slen, p_doff, p_dcap, base(n);
  std::vector<ZhBgzfMember> mem;
  std::vector<ZhBgzfTask> tasks;
  std::vector<uint32_t> mfirst(n + 1);
  std::vector<size_t> piece_member;
  uint64_t slots_total = 0, out_total = 0;
  for (size_t i = 0; i < n; i++) {
    mfirst[i] = (uint32_t)mem.size();
    base[i] = out_total;
    for (uint64_t o = 0; o < slen[i]; o += bb) {
      const uint64_t len = std::min<uint64_t>(bb, slen[i] - o);
      // (a piece whose worst case fits a member needs no more than that)
      const uint64_t cap = std::min<uint64_t>(ZH_BGZF_MAX_CDATA, zh_compress_bound(len, ZH_DF_DEFLATE));
      piece_member.push_back(mem.size());
      for (uint32_t lo = 0; lo == 0 || lo < cap; lo += kTaskBytes) tasks.push_back(ZhBgzfTask{(uint32_t)mem.size(), lo});
      mem.push_back(ZhBgzfMember{slots_total, base[i], mfirst[i], (uint32_t)p_soff.size(), (uint32_t)cap, (uint32_t)len, 0, 0});
      p_soff.push_back(soff[i] + o);
      p_slen.push_back(len);
      p_doff.push_back(slots_total);
      p_dcap.push_back(cap);
      slots_total += (cap + kGatherSlack + 255) & ~(uint64_t)255;
      out_total += 26 + cap;
    }
    tasks.push_back(ZhBgzfTask{(uint32_t)mem.size(), 0});
    mem.push_back(ZhBgzfMember{0, base[i], mfirst[i], 0, 0, 0, 2, 0});
    out_total = (out_total + 28 + 255) & ~(uint64_t)255;
    if (mem.size() >= 0x7fffffffull || tasks.size() >= 0x7fffffffull) return ZH_ERR_ARGUMENT;
  }
  mfirst[n] = (uint32_t)mem.size();
  const size_t n_piece = p_soff.size(), n_mem = mem.size(), n_task = tasks.size();

  // ---- 2. one compress plan; the pieces that outgrew a member once more at level 0 ----
  DevBuf d_slots0, d_slots1;
  PlanGuard pg0, pg1;
  std::vector<uint64_t> clen(n_piece);
  std::vector<int32_t> cst(n_piece);
  if (dev_alloc(ctx, d_slots0, slots_total + 256) != hipSuccess) return ZH_ERR_NOMEM;
  if (n_piece) {
    if ((st = zh_plan_compress(ctx, n_piece, p_soff.data(), p_slen.data(), p_doff.data(), p_dcap.data(), level,
                               ZH_DF_DEFLATE, &pg0.p)) ||
        (st = zh_plan_request_crc32(pg0.p, 1)) || (st = zh_plan_run(pg0.p, d_src.p, d_slots0.p)) ||
        (st = zh_plan_results(pg0.p, clen.data(), cst.data())))
      return st;
  }
  std::vector<size_t> redo;
  for (size_t k = 0; k < n_piece; k++)
    if (cst[k] == ZH_ERR_DST_TOO_SMALL) redo.push_back(k);
  if (!redo.empty()) {
    const size_t nr = redo.size();
    std::vector<uint64_t> r_soff(nr), r_slen(nr), r_doff(nr), r_dcap(nr), r_len(nr);
    std::vector<int32_t> r_st(nr);
    uint64_t total1 = 0;
    for (size_t q = 0; q < nr; q++) {
      ZhBgzfMember& m = mem[piece_member[redo[q]]];
      r_soff[q] = p_soff[redo[q]];
      r_slen[q] = p_slen[redo[q]];
      r_doff[q] = total1;
      r_dcap[q] = 5 + r_slen[q];  // one stored block
      m.slot = total1;
      m.idx = (uint32_t)q;
      m.cap = (uint32_t)r_dcap[q];
      m.which = 1;
      total1 += (r_dcap[q] + kGatherSlack + 255) & ~(uint64_t)255;
    }
    if (dev_alloc(ctx, d_slots1, total1 + 256) != hipSuccess) return ZH_ERR_NOMEM;
    if ((st = zh_plan_compress(ctx, nr, r_soff.data(), r_slen.data(), r_doff.data(), r_dcap.data(), ZH_NO_COMPRESSION,
                               ZH_DF_DEFLATE, &pg1.p)) ||
        (st = zh_plan_request_crc32(pg1.p, 1)) || (st = zh_plan_run(pg1.p, d_src.p, d_slots1.p)) ||
        (st = zh_plan_results(pg1.p, r_len.data(), r_st.data())))
      return st;
    for (size_t q = 0; q < nr; q++) cst[redo[q]] = r_st[q];
  }
  tr.mark(ctx, "bgzf write: compress");

  // ---- 3. sizes, places, every byte of every image ----
  const ZhBgzfMember* d_mem;
  const ZhBgzfTask* d_tasks;
  const uint32_t* d_mfirst;
  uint32_t* d_msize;
  uint64_t *d_mpos, *d_ilen;
  Arena ar;
  ar.add(d_mem, n_mem, mem.data());
  ar.add(d_tasks, n_task, tasks.data());
  ar.add(d_mfirst, n + 1, mfirst.data());
  const size_t ar_in = ar.size;  // (what is uploaded: the arrays so far)
  ar.add(d_msize, n_mem);
  ar.add(d_mpos, n_mem + 1);
  ar.add(d_ilen, n);
  DevBuf d_ar, d_out;
  if (ar.alloc(ctx, d_ar, 256) != hipSuccess || dev_alloc(ctx, d_out, out_total + 256) != hipSuccess) return ZH_ERR_NOMEM;
  ar.bind();
  {
    std::vector<uint8_t> h(ar_in);
    ar.gather(h.data());
    const void* src = h.data();
    if ((st = zhh_upload_slices(ctx, &src, {0}, {(uint64_t)ar_in}, ar_in, ar.base))) return st;
  }
  const uint64_t* const len0 = n_piece ? zh_plan_device_lens(pg0.p) : nullptr;
  const uint64_t* const len1 = pg1.p ? zh_plan_device_lens(pg1.p) : nullptr;
  const uint32_t* const crc0 = n_piece ? pg0.p->buf_crc : nullptr;
  const uint32_t* const crc1 = pg1.p ? pg1.p->buf_crc : nullptr;
  const uint8_t *const slots0 = d_slots0.p, *const slots1 = d_slots1.p;
  uint8_t* const outp = d_out.p;
  hipLaunchKernelGGL(zh_bgzf_sizes_kernel, dim3(((uint32_t)n_mem + 255) / 256), wg, 0, s, d_mem, (uint32_t)n_mem, len0,
                     len1, d_msize);
  hipLaunchKernelGGL(zh_bgzf_scan64_kernel, dim3(1), wg, 0, s, (const uint32_t*)d_msize, (uint32_t)n_mem, d_mpos);
  hipLaunchKernelGGL(zh_bgzf_image_len_kernel, dim3(((uint32_t)n + 255) / 256), wg, 0, s, d_mfirst, (uint32_t)n,
                     (const uint64_t*)d_mpos, d_ilen);
  hipLaunchKernelGGL(zh_bgzf_assemble_kernel, dim3(((uint32_t)n_task + 3) / 4), wg, 0, s, slots0, slots1, outp, d_mem,
                     d_tasks, (uint32_t)n_task, (const uint64_t*)d_mpos, len0, len1, crc0, crc1);
  ZH_HIP(ctx, hipGetLastError());
  std::vector<uint64_t> ilen(n);
  ZH_HIP(ctx, hipMemcpyAsync(ilen.data(), d_ilen, n * 8, hipMemcpyDeviceToHost, s));
  ZH_HIP(ctx, hipStreamSynchronize(s));
  tr.mark(ctx, "bgzf write: assemble");

  // ---- 4. the images: an image with a piece that failed is not handed out ----
  std::vector<size_t> pos(n);
  std::vector<int32_t> ist(n, ZH_OK);
  for (size_t i = 0, k = 0; i < n; i++) {
    pos[i] = i;
    for (uint32_t m = mfirst[i]; m + 1 < mfirst[i + 1]; m++, k++)
      if (ist[i] == ZH_OK && cst[k] != ZH_OK) ist[i] = cst[k];
  }
  if ((st = writer_hand_out(ctx, d_out.p, pos, base, ilen, ist, dsts, dst_lens, statuses))) {
    clear_outputs(dsts, dst_lens, statuses, n);
    return st;
  }
  tr.mark(ctx, "bgzf write: download");
  return ZH_OK;
}

extern "C" int zh_bgzf_index_batch(zh_ctx* ctx, const void* const* images, const size_t* lens, size_t n,
                                   zh_bgzf_entry** index, size_t* first, int32_t* statuses, uint8_t* has_eof) {
  if (!ctx || !index || !first || (n && (!images || !lens || !statuses))) return ZH_ERR_ARGUMENT;
  *index = nullptr;
  for (size_t t = 0; t <= n; t++) first[t] = 0;
  for (size_t t = 0; t < n; t++) {
    statuses[t] = ZH_OK;
    if (has_eof) has_eof[t] = 0;
  }
  if (const int e = images_there(images, lens, n)) return e;
  if (!n) return ZH_OK;
  Trace tr;
  BgzfWalk W;
  if (const int st = bgzf_walk(ctx, tr, images, lens, n, W)) return st;
  size_t total = 0;
  std::vector<int32_t> wst(n);
  for (size_t t = 0; t < n; t++) {
    wst[t] = W.walk_status(t);
    if (wst[t] == ZH_OK) total += W.rec_ranges[2 * t + 1] - W.rec_ranges[2 * t] + 1;
  }
  zh_bgzf_entry* e = (zh_bgzf_entry*)malloc((total ? total : 1) * sizeof(zh_bgzf_entry));
  if (!e) return ZH_ERR_NOMEM;
  size_t at = 0;
  for (size_t t = 0; t < n; t++) {
    first[t] = at;
    statuses[t] = wst[t];
    if (has_eof) has_eof[t] = W.has_eof(t);
    if (wst[t] != ZH_OK) continue;
    uint64_t end = 0, utotal = 0;
    for (uint32_t r = W.rec_ranges[2 * t]; r < W.rec_ranges[2 * t + 1]; r++) {
      const ZhBgzfRec& m = W.recs[r];
      e[at++] = zh_bgzf_entry{m.coff, m.uoff};
      end = m.cdata_off + m.cdata_len + 8;
      utotal = m.uoff + m.isize;
    }
    e[at++] = zh_bgzf_entry{end, utotal};
  }
  first[n] = at;
  *index = e;
  return ZH_OK;
}

extern "C" int zh_bgzf_read_batch(zh_ctx* ctx, const void* const* images, const size_t* lens, size_t n, void** dsts,
                                  size_t* dst_lens, int32_t* statuses, uint8_t* has_eof) {
  if (!ctx || (n && (!images || !lens || !dsts || !dst_lens || !statuses))) return ZH_ERR_ARGUMENT;
  clear_outputs(dsts, dst_lens, statuses, n);
  for (size_t t = 0; has_eof && t < n; t++) has_eof[t] = 0;
  if (const int e = images_there(images, lens, n)) return e;
  if (!n) return ZH_OK;
  Trace tr;
  int st;
  BgzfWalk W;
  if ((st = bgzf_walk(ctx, tr, images, lens, n, W))) return st;
  hipStream_t s = ctx->stream;
  const uint32_t n_img = (uint32_t)n, n_rec = W.n_rec;

  // ---- the layout of the output: member k of an image at the prefix sum of the ISIZEs before it ----
  std::vector<uint64_t> aoff(n), alen(n, 0), p_soff, p_slen, p_doff, p_dcap;
  std::vector<uint32_t> pidx(n_rec, kNone);
  uint64_t out_total = 0;
  for (size_t t = 0; t < n; t++) {
    aoff[t] = out_total;
    for (uint32_t r = W.rec_ranges[2 * t]; r < W.rec_ranges[2 * t + 1]; r++) {
      const ZhBgzfRec& m = W.recs[r];
      if (m.status != ZH_OK) continue;
      pidx[r] = (uint32_t)p_soff.size();
      p_soff.push_back(W.S.up_off[t] + m.cdata_off);
      p_slen.push_back(m.cdata_len);
      p_doff.push_back(aoff[t] + m.uoff);
      p_dcap.push_back(m.isize);
      alen[t] = m.uoff + m.isize;
    }
    out_total = (out_total + alen[t] + 255) & ~(uint64_t)255;
  }

  // ---- one decode, every verdict, the first failure of every image ----
  const uint32_t* d_pidx;
  int32_t* d_est;
  uint32_t *d_bad, *d_any;
  Arena ar;
  ar.add(d_est, n_rec);
  ar.add(d_bad, n_img);
  const size_t ar_out = ar.size;  // (what comes back: the arrays so far, in one copy)
  ar.add(d_pidx, n_rec, pidx.data());
  ar.add(d_any, n_img);
  DevBuf d_ar, d_out;
  if (ar.alloc(ctx, d_ar, 256) != hipSuccess || dev_alloc(ctx, d_out, out_total + 256) != hipSuccess) return ZH_ERR_NOMEM;
  ar.bind();
  ZH_HIP(ctx, ar.upload(s));
  ZH_HIP(ctx, hipStreamSynchronize(s));  // (pidx is the scope's)
  PlanGuard pg;
  if ((st = decode_and_verify(ctx, W.S.d_in.p, d_out.p, p_soff, p_slen, p_doff, p_dcap, W.d_recs, d_pidx, n_rec, d_est, pg)))
    return st;
  const uint32_t* const d_rr = W.d_rec_ranges;  // (a plain pointer: a launch must not take the walk's buffers along)
  hipLaunchKernelGGL(zh_zip_reduce_kernel, dim3(n_img), dim3(256), 0, s, d_rr, (const int32_t*)d_est, (const uint8_t*)nullptr, d_bad, d_any);
  ZH_HIP(ctx, hipGetLastError());
  std::vector<uint8_t> h_ar;
  if ((st = fetch(ctx, h_ar, ar, 0, ar_out))) return st;
  const int32_t* const est = ar.host(h_ar.data(), (const int32_t*)d_est);
  const uint32_t* const bad = ar.host(h_ar.data(), (const uint32_t*)d_bad);
  tr.mark(ctx, "bgzf read: decode + verify");

  std::vector<int32_t> ist(n);
  for (size_t t = 0; t < n; t++)
    ist[t] = W.start[t] != ZH_OK ? W.start[t] : bad[t] != kNone ? est[bad[t]] : (int32_t)ZH_OK;
  if ((st = hand_out(ctx, d_out.p, aoff, alen, ist, dsts, dst_lens, statuses))) return st;
  for (size_t t = 0; has_eof && t < n; t++) has_eof[t] = W.has_eof(t);
  tr.mark(ctx, "bgzf read: download");
  return ZH_OK;
}

// ---------------------------------------------------------------------------
// range reads
// ---------------------------------------------------------------------------
namespace {

// What can be said of an index without looking at the image: at least the closing entry, entry 0 at byte 0, neither
// offset ever falling, no member of more than 65536 bytes, nothing beyond the image
bool bgzf_index_sound(const zh_bgzf_entry* e, size_t n, uint64_t image_len) {
  if (n < 1 || n > 0x7ffffffeull || e[0].uoff != 0) return false;
  for (size_t k = 0; k < n; k++) {
    if (e[k].coff > image_len) return false;
    if (k + 1 < n && (e[k + 1].coff < e[k].coff || e[k + 1].uoff < e[k].uoff || e[k + 1].uoff - e[k].uoff > 65536))
      return false;
  }
  return true;
}

}  // namespace

extern "C" int zh_bgzf_read_ranges(zh_ctx* ctx, const void* const* images, const size_t* lens, size_t n_images,
                                   const zh_bgzf_entry* index, const size_t* first, size_t n_ranges,
                                   const uint64_t* range_image, const uint64_t* range_off, const uint64_t* range_len,
                                   void** dsts, size_t* dst_lens, int32_t* statuses) {
  if (!ctx || (n_images && (!images || !lens)) || (n_ranges && (!dsts || !dst_lens || !statuses))) return ZH_ERR_ARGUMENT;
  clear_outputs(dsts, dst_lens, statuses, n_ranges);
  if (const int e = images_there(images, lens, n_images)) return e;
  if (n_ranges > 0x7fffffffull) return ZH_ERR_ARGUMENT;

  // ---- 1. pread's arithmetic and the binary search (zh_range_host.h) ----
  std::vector<RangeGeo> geo;
  if (const int e = range_geometry(
          n_images, index, first, n_ranges, range_image, range_off, range_len,
          [&](size_t t, const zh_bgzf_entry* e, size_t ne) { return bgzf_index_sound(e, ne, lens[t]); },
          [](const zh_bgzf_entry& x) { return x.uoff; }, geo))
    return e;
  if (!n_ranges) return ZH_OK;
  Trace tr;

  // ---- 2. the spans [coff[k0], coff[k1 + 1]), merged image by image; one upload ----
  RangeSpans up;
  for (size_t r = 0; r < n_ranges; r++) {
    const RangeGeo& q = geo[r];
    if (q.fixed != ZH_OK || q.k0 > q.k1) continue;
    const zh_bgzf_entry* e = index + first[range_image[r]];
    up.add(range_image[r], e[q.k0].coff, e[q.k1 + 1].coff);
  }
  up.place(images);
  const uint64_t up_total = up.up_total;
  ZH_HIP(ctx, hipSetDevice(ctx->device));
  int st;
  hipStream_t s = ctx->stream;
  const dim3 wg(256);
  DevBuf d_src;
  if (dev_alloc(ctx, d_src, up_total + 512) != hipSuccess) return ZH_ERR_NOMEM;
  if ((st = zhh_upload_slices(ctx, up.sp.data(), up.soff, up.slen, up_total, d_src.p))) return st;
  tr.mark(ctx, "bgzf ranges: upload");

  // ---- 3. the touched members: where they are in the upload, what the index promises; slots, scratch, clips ----
  std::vector<uint64_t> m_at, m_doff, doff(n_ranges), dcap(n_ranges);
  std::vector<uint32_t> m_avail, m_want, m_ranges(2 * n_ranges, 0);
  std::vector<char> m_edge;
  std::vector<ZhClipDesc> clips;
  uint64_t dst_total = 0, scratch = 0;
  for (size_t r = 0; r < n_ranges; r++) {
    doff[r] = dst_total;
    dcap[r] = geo[r].end - geo[r].off;
    dst_total += (dcap[r] + 255) & ~(uint64_t)255;
  }
  const uint64_t scratch_base = dst_total;
  for (size_t r = 0; r < n_ranges; r++) {
    const RangeGeo& q = geo[r];
    m_ranges[2 * r] = m_ranges[2 * r + 1] = (uint32_t)m_at.size();
    if (q.fixed != ZH_OK || q.k0 > q.k1) continue;
    const uint64_t t = range_image[r];
    const zh_bgzf_entry* e = index + first[t];
    const RangeSpans::Span& x = up.holding(t, e[q.k0].coff);
    if (m_at.size() + (q.k1 - q.k0 + 1) > 0x7fffffffull) return ZH_ERR_ARGUMENT;
    for (size_t k = q.k0; k <= q.k1; k++) {
      const uint64_t bs = e[k].uoff, be = e[k + 1].uoff;
      if (be == bs) continue;  // (an empty member: nothing of it lies in any range)
      m_at.push_back(x.dev + (e[k].coff - x.lo));
      m_avail.push_back((uint32_t)std::min<uint64_t>(e[k + 1].coff - e[k].coff, 0x7fffffffu));
      m_want.push_back((uint32_t)(be - bs));
      if (bs >= q.off && be <= q.end) {
        m_edge.push_back(0);
        m_doff.push_back(doff[r] + (bs - q.off));
        continue;
      }
      m_edge.push_back(1);
      m_doff.push_back(scratch_base + scratch);
      const uint64_t lo = std::max(q.off, bs), hi = std::min(q.end, be);
      append_clips(clips, scratch + (lo - bs), doff[r] + (lo - q.off), hi - lo);
      scratch += (be - bs + kGatherSlack + 255) & ~(uint64_t)255;
    }
    m_ranges[2 * r + 1] = (uint32_t)m_at.size();
    if (clips.size() > 0x7fffffffull) return ZH_ERR_ARGUMENT;
  }
  const size_t n_mem = m_at.size();
  const uint32_t n_rng = (uint32_t)n_ranges;

  // ---- 4. the headers, parsed on the device; their records come back for the plan ----
  const uint64_t* d_at;
  const uint32_t *d_avail, *d_want, *d_mr;
  const ZhClipDesc* d_clips;
  ZhBgzfRec* d_recs;
  uint32_t *d_pidx, *d_bad, *d_any;
  int32_t* d_est;
  Arena ar;
  ar.add(d_recs, n_mem);
  const size_t ar_recs = ar.size;  // (what comes back: first the records, later the verdicts too, a copy each)
  ar.add(d_est, n_mem);
  ar.add(d_bad, n_ranges);
  const size_t ar_out = ar.size;
  ar.add(d_at, n_mem, m_at.data());
  ar.add(d_avail, n_mem, m_avail.data());
  ar.add(d_want, n_mem, m_want.data());
  ar.add(d_mr, 2 * n_ranges, m_ranges.data());
  ar.add(d_clips, clips.size(), clips.data());
  ar.add(d_pidx, n_mem);
  ar.add(d_any, n_ranges);
  DevBuf d_ar, d_dst;
  if (ar.alloc(ctx, d_ar, 256) != hipSuccess || dev_alloc(ctx, d_dst, dst_total + scratch + 256) != hipSuccess)
    return ZH_ERR_NOMEM;
  ar.bind();
  ZH_HIP(ctx, ar.upload(s));
  const uint8_t* const in = d_src.p;
  uint8_t* const outp = d_dst.p;
  if (n_mem)
    hipLaunchKernelGGL(zh_bgzf_parse_at_kernel, dim3(((uint32_t)n_mem + 255) / 256), wg, 0, s, in, d_at, d_avail, d_want,
                       (uint32_t)n_mem, d_recs);
  ZH_HIP(ctx, hipGetLastError());
  std::vector<uint8_t> h_recs, h_ar;
  if ((st = fetch(ctx, h_recs, ar, 0, ar_recs))) return st;
  const ZhBgzfRec* const recs = ar.host(h_recs.data(), (const ZhBgzfRec*)d_recs);
  std::vector<uint64_t> p_soff, p_slen, p_doff, p_dcap;
  std::vector<uint32_t> pidx(n_mem, kNone);
  uint64_t in_place = 0, via_scratch = 0;
  for (size_t m = 0; m < n_mem; m++) {
    if (recs[m].status != ZH_OK) continue;
    pidx[m] = (uint32_t)p_soff.size();
    p_soff.push_back(recs[m].cdata_off);
    p_slen.push_back(recs[m].cdata_len);
    p_doff.push_back(m_doff[m]);
    p_dcap.push_back(m_want[m]);
    (m_edge[m] ? via_scratch : in_place)++;
  }
  if (n_mem) ZH_HIP(ctx, hipMemcpyAsync(d_pidx, pidx.data(), n_mem * 4, hipMemcpyHostToDevice, s));
  ZH_HIP(ctx, hipStreamSynchronize(s));  // (pidx is the scope's)
  tr.mark(ctx, "bgzf ranges: headers");

  // ---- 5. one decode, every verdict, the clips, the lowest failing member of every range ----
  PlanGuard pg;
  if ((st = decode_and_verify(ctx, in, outp, p_soff, p_slen, p_doff, p_dcap, d_recs, d_pidx, (uint32_t)n_mem, d_est, pg)))
    return st;
  zh_launch_range_clip(s, outp + scratch_base, outp, d_clips, (uint32_t)clips.size());
  hipLaunchKernelGGL(zh_zip_reduce_kernel, dim3(n_rng), wg, 0, s, d_mr, (const int32_t*)d_est, (const uint8_t*)nullptr,
                     d_bad, d_any);
  ZH_HIP(ctx, hipGetLastError());
  if ((st = fetch(ctx, h_ar, ar, ar_recs, ar_out))) return st;
  const int32_t* const est = ar.host(h_ar.data(), (const int32_t*)d_est);
  const uint32_t* const bad = ar.host(h_ar.data(), (const uint32_t*)d_bad);
  ctx->rg_uploaded = up_total;
  ctx->rg_in_place = in_place;
  ctx->rg_via_scratch = via_scratch;
  tr.mark(ctx, "bgzf ranges: decode");

  std::vector<int32_t> rst(n_ranges);
  for (size_t r = 0; r < n_ranges; r++)
    rst[r] = geo[r].fixed != ZH_OK ? geo[r].fixed : bad[r] != kNone ? est[bad[r]] : (int32_t)ZH_OK;
  if ((st = hand_out(ctx, d_dst.p, doff, dcap, rst, dsts, dst_lens, statuses))) return st;
  tr.mark(ctx, "bgzf ranges: download");
  return ZH_OK;
}
