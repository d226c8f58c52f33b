// Any gzip file (RFC 1952): a series of members, each a header with optional FEXTRA, FNAME, FCOMMENT and FHCRC fields,
// a raw-deflate stream and a trailer of CRC-32 and ISIZE -- cat a.gz b.gz, appended logs, pigz -i, .warc.gz.  Unlike
// a BGZF member (zh_bgzf.hip) a plain member does not say how long it is: where member k + 1 starts is known only once
// member k's deflate stream has been decoded to its end.  So every position that could start a member is sized at
// once, as if one started there, and the chain from byte 0 is proved afterwards (zh_walk.h), the way zh_inflate_seg.hip
// guesses block starts and the four batch readers walk their records.
//   zh_sig_scan_kernel        the positions that hold 1f 8b 08 and a FLG without a reserved bit (zh_scan.h)
//   zh_gzip_ranges_kernel     per image: its hits; what stands at byte 0 when that is no hit
//   zh_gzip_head_kernel       a wave a candidate: the header checks, the fields' places, the deflate stream's source
//   zh_inflate_tokens_kernel<.., kCount, kRec>   the SPECULATIVE SIZING PASS (zh_inflate_split.hip): every candidate
//                             whose header parsed is decoded without writing anything -- its output bytes and the bit
//                             behind its final block --, under a budget of input bytes the call's workgroups share
//   zh_gzip_next_kernel       where the member at a hit ends, that position found among the hits
//   zh_walk_double / scan     the hits reachable from byte 0 ARE the members
//   zh_gzip_frontier_kernel   the reached candidates the budget left unresolved: those, all of them real members, are
//                             sized without a budget, and next and the walk run again -- until no chain ends at one
//   zh_gzip_tail_kernel       an image whose chain stops where no member starts: are the bytes behind it all zero?
//   zh_gzip_parse_kernel      one zh_gzip_member a reached member; zh_gzip_scan64 / uoff: its place in the data
// Reading: ONE raw-deflate uncompress plan over every reached member, sources in place, each slot the size the sizing
// pass found, CRC-32 requested; the headers that carry FHCRC go through the checksum kernels as buffers of their own;
//   zh_gzip_verify_kernel     header, decoder, FHCRC, CRC-32, ISIZE, what stands behind the member -- the first that fails
//   zh_zip_reduce_kernel      per image: the first member that failed, in file order
// The host parses no header byte, compares no checksum and copies no payload byte.
#include "zh_range_host.h"
#include "zh_scan.h"
#include "zh_zip_dev.h"

namespace {

struct GzipSignature {  // ID1, ID2, CM = 8, a FLG with no reserved bit
  static __device__ __forceinline__ bool match(uint32_t v) { return (v & 0xe0ffffffu) == 0x00088b1fu; }
};

constexpr int32_t kUnresolved = -1;  // succ[]: the member at this node was not sized (the budget)
constexpr int32_t kHeadOpen = -3;    // a header's status: its NUL search was given up (the budget)
constexpr uint64_t kNulGivenUp = ~0ull;
constexpr uint64_t kNulStride = 4096;  // bytes of a NUL search between two payments
// The budget of input bytes that the header kernel's NUL searches and the sizing pass share (null: none)
struct GzipBudget {
  unsigned long long* used;
  uint64_t budget;
};
constexpr int32_t kAskTail = -2;     // succ[]: no hit where the member ends -- zeros to the image's end, or garbage?

// What the header checks leave of a candidate; offsets count from the candidate's first byte
struct ZhGzipHead {
  uint64_t cdata_off;
  int32_t status;
  uint32_t mtime;
  uint32_t flg, xfl, os;
  uint32_t extra_off, extra_len, name_off, name_len, comment_off, comment_len;
  uint32_t hcrc_off;  // FHCRC's two bytes (0: none)
};
// What the host needs of a reached member beside its zh_gzip_member
struct ZhGzipAux {
  int32_t status;       // the header's, then the decoder's
  int32_t succ_status;  // what stands behind the member
  uint32_t hcrc_off, pad;
};

// the checks that need no field: what stands at a position that the scan did not find (pos <= len)
__device__ __forceinline__ int32_t quick_status(const uint8_t* __restrict__ p, uint64_t len, uint64_t pos) {
  if (len - pos < 18) return ZH_ERR_INVALID_BUFFER;
  const uint8_t* __restrict__ q = p + pos;
  if (q[0] != 0x1f || q[1] != 0x8b) return ZH_ERR_GZIP_ID;
  if (q[2] != 8) return ZH_ERR_UNSUPPORTED_METHOD;
  if (q[3] & 0xe0u) return ZH_ERR_RESERVED_FLAGS;
  return ZH_OK;
}

// The first NUL of q[from, left), by the whole wave: 64 bytes a step, one ballot.  `left` if there is none.  A false
// candidate's "name" can run for megabytes, and an image without a zero byte can hold one every four bytes: every
// kNulStride bytes lane 0 pays them into the call's counter, and a search that finds the budget spent is given up
// (kNulGivenUp), as is one that starts with it spent.  A name shorter than that -- every real one -- pays nothing.
__device__ __forceinline__ uint64_t find_nul(const uint8_t* __restrict__ q, uint64_t from, uint64_t left, uint32_t lane,
                                             GzipBudget bd) {
  for (uint64_t at = from; at < left; at += 64) {
    if (bd.used && ((at - from) & (kNulStride - 1)) == 0) {  // (a search that starts with the budget spent pays nothing)
      uint32_t over = 0;
      if (lane == 0)
        over = (at == from ? *(volatile unsigned long long*)bd.used
                           : atomicAdd(bd.used, (unsigned long long)kNulStride) + kNulStride) >= bd.budget ? 1u : 0u;
      if (__shfl((int)over, 0)) return kNulGivenUp;
    }
    const bool z = at + lane < left && q[at + lane] == 0;
    const uint64_t m = __ballot(z);
    if (m) return at + (uint32_t)__builtin_ctzll(m);
  }
  return left;
}

// the member header at position pos of an image of len bytes (pos <= len), by one wave; every lane gets the record
__device__ __forceinline__ ZhGzipHead head_at(const uint8_t* __restrict__ p, uint64_t len, uint64_t pos, uint32_t lane,
                                              GzipBudget bd) {
  ZhGzipHead h{};
  h.status = quick_status(p, len, pos);
  if (h.status != ZH_OK) return h;
  const uint64_t left = len - pos;
  const uint8_t* __restrict__ q = p + pos;
  h.flg = q[3];
  h.mtime = ld32(q + 4);
  h.xfl = q[8];
  h.os = q[9];
  uint64_t off = 10;
  auto fail = [&]() {
    h.status = ZH_ERR_INVALID_BUFFER;
    return h;
  };
  auto open = [&]() {
    h.status = kHeadOpen;
    return h;
  };
  if (h.flg & 4u) {  // FEXTRA (12 <= left: no member is shorter than 18 bytes)
    const uint32_t xlen = ld16(q + 10);
    if (12ull + xlen > left) return fail();
    h.extra_off = 12;
    h.extra_len = xlen;
    off = 12ull + xlen;
  }
  if (h.flg & 8u) {  // FNAME
    const uint64_t z = find_nul(q, off, left, lane, bd);
    if (z == kNulGivenUp) return open();
    if (z == left) return fail();
    h.name_off = (uint32_t)off;
    h.name_len = (uint32_t)(z - off);
    off = z + 1;
  }
  if (h.flg & 16u) {  // FCOMMENT
    const uint64_t z = find_nul(q, off, left, lane, bd);
    if (z == kNulGivenUp) return open();
    if (z == left) return fail();
    h.comment_off = (uint32_t)off;
    h.comment_len = (uint32_t)(z - off);
    off = z + 1;
  }
  if (h.flg & 2u) {  // FHCRC: verified once the member is reached
    if (off + 2 > left) return fail();
    h.hcrc_off = (uint32_t)off;
    off += 2;
  }
  if (off > 0xffffffffull) return fail();  // (the fields' places are 32 bits wide: no header of 4 GiB)
  h.cdata_off = off;
  return h;
}

}  // namespace

// ---------------------------------------------------------------------------
// the candidates
// ---------------------------------------------------------------------------
// Per image: ranges[2t .. 2t + 1] = its hits; start[t] = ZH_OK when its byte 0 is a hit or it is empty, else what
// the checks say of byte 0
__global__ __launch_bounds__(256) void zh_gzip_ranges_kernel(const uint8_t* __restrict__ d_in,
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
    st = quick_status(d_in + g.up_off, g.len, 0);
    if (st == ZH_OK) st = ZH_ERR_INVALID_BUFFER;  // (cannot be: such a position is a hit)
  }
  start[t] = st;
}

// a candidate's deflate stream as a source of the sizing pass: in place, bounded by the image's end minus the
// trailer's 8 bytes
__device__ __forceinline__ ZhBufDesc source_of(const ZhZrImg& g, uint64_t at, const ZhGzipHead& h) {
  ZhBufDesc d{};
  const uint64_t from = at - g.up_off + h.cdata_off;
  d.src_off = at + h.cdata_off;
  d.src_len = h.status == ZH_OK && g.len >= 8 && from < g.len - 8 ? g.len - 8 - from : 0;
  return d;
}

// One wave per candidate (four a workgroup): its header's record and its source; a candidate whose header failed or
// was left open is no stream (status != ZH_OK: the pass leaves it alone).
__global__ __launch_bounds__(256) void zh_gzip_head_kernel(const uint8_t* __restrict__ d_in,
                                                           const ZhZrImg* __restrict__ imgs, uint32_t n_img,
                                                           const uint64_t* __restrict__ hits, uint32_t n_hits,
                                                           GzipBudget bd, ZhGzipHead* __restrict__ heads,
                                                           ZhBufDesc* __restrict__ bufs, int32_t* __restrict__ dec_st,
                                                           uint32_t* __restrict__ body_pos) {
  const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = zh_lane();
  if (b >= n_hits) return;
  const uint64_t at = hits[b];
  const ZhZrImg g = imgs[find_img(imgs, n_img, at)];
  const ZhGzipHead h = head_at(d_in + g.up_off, g.len, at - g.up_off, lane, bd);
  if (lane != 0) return;
  heads[b] = h;
  bufs[b] = source_of(g, at, h);
  dec_st[b] = h.status;
  body_pos[b] = 0;
}

// next[b] for every node b: nodes [0, n_hits) are the hits, node n_hits + t is image t's END (its own successor).  A
// hit's successor is the hit where its member ends; it is END when the member fails (header or decoder), when it was
// not sized (succ = kUnresolved), when it ends where the image ends, and when that position is no hit (succ =
// kAskTail: zh_gzip_tail_kernel decides).  mend[b]: the position behind the member.  mark[b] = 1 for byte 0 of an image.
__global__ __launch_bounds__(256) void zh_gzip_next_kernel(const ZhZrImg* __restrict__ imgs, uint32_t n_img,
                                                           const uint64_t* __restrict__ hits, uint32_t n_hits,
                                                           const uint32_t* __restrict__ ranges,
                                                           const ZhGzipHead* __restrict__ heads,
                                                           const int32_t* __restrict__ dec_st,
                                                           const uint64_t* __restrict__ end_bit,
                                                           const uint32_t* __restrict__ unres, uint32_t n_nodes,
                                                           uint32_t* __restrict__ jump, uint32_t* __restrict__ mark,
                                                           int32_t* __restrict__ succ, uint64_t* __restrict__ mend) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n_nodes) return;
  uint32_t nx = b, mk = 0;
  if (b < n_hits) {
    const uint64_t at = hits[b];
    const uint32_t t = find_img(imgs, n_img, at);
    const ZhZrImg g = imgs[t];
    const uint64_t pos = at - g.up_off;
    int32_t sc = ZH_OK;
    uint64_t end = 0;
    nx = n_hits + t;
    if (heads[b].status == kHeadOpen || (heads[b].status == ZH_OK && unres[b])) {
      sc = kUnresolved;
    } else if (heads[b].status == ZH_OK && dec_st[b] == ZH_OK) {
      end = pos + heads[b].cdata_off + ((end_bit[b] + 7) >> 3) + 8;
      if (end > g.len) {
        sc = ZH_ERR_INVALID_BUFFER;  // (the stream's input ends 8 bytes before the image does: cannot be)
      } else if (end != g.len) {
        const uint32_t hi = ranges[2 * t + 1], k = lower_bound(hits, b + 1, hi, g.up_off + end);
        if (k < hi && hits[k] == g.up_off + end)
          nx = k;
        else
          sc = kAskTail;
      }
    }
    succ[b] = sc;
    mend[b] = end;
    mk = pos == 0 ? 1u : 0u;
  }
  jump[b] = nx;
  mark[b] = mk;
}

// The frontier: the reached candidates that were not sized -- a chain's end each, so about one an image --, gathered
// in any order: front[k] = the node; *count: how many they are.
__global__ __launch_bounds__(256) void zh_gzip_frontier_kernel(const uint32_t* __restrict__ mark,
                                                               const int32_t* __restrict__ succ, uint32_t n_hits,
                                                               uint32_t* __restrict__ front, uint32_t* __restrict__ count) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n_hits) return;
  if (!mark[b] || succ[b] != kUnresolved) return;
  front[atomicAdd(count, 1u)] = b;
}
// ... and made the streams of a sizing pass of their own, without a budget, one wave each: a header that was left
// open is read to its end first; fbufs[k] = the source, f_st[k] = the header's status.
__global__ __launch_bounds__(256) void zh_gzip_front_head_kernel(const uint8_t* __restrict__ d_in,
                                                                 const ZhZrImg* __restrict__ imgs, uint32_t n_img,
                                                                 const uint64_t* __restrict__ hits,
                                                                 const uint32_t* __restrict__ front, uint32_t n_front,
                                                                 ZhGzipHead* __restrict__ heads, ZhBufDesc* __restrict__ bufs,
                                                                 ZhBufDesc* __restrict__ fbufs, int32_t* __restrict__ f_st,
                                                                 uint64_t* __restrict__ f_out, uint64_t* __restrict__ f_end,
                                                                 uint32_t* __restrict__ f_unres) {
  const uint32_t k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = zh_lane();
  if (k >= n_front) return;
  const uint32_t b = front[k];
  const uint64_t at = hits[b];
  const ZhZrImg g = imgs[find_img(imgs, n_img, at)];
  ZhGzipHead h = heads[b];
  const bool open = h.status == kHeadOpen;  // (the same in every lane)
  if (open) h = head_at(d_in + g.up_off, g.len, at - g.up_off, lane, GzipBudget{nullptr, 0});
  if (lane != 0) return;
  if (open) {
    heads[b] = h;
    bufs[b] = source_of(g, at, h);
  }
  fbufs[k] = bufs[b];
  f_st[k] = h.status;
  f_out[k] = 0;
  f_end[k] = 0;
  f_unres[k] = 0;
}
// ... and what that pass found goes back to the candidates' own arrays
__global__ __launch_bounds__(256) void zh_gzip_settle_kernel(const uint32_t* __restrict__ front, uint32_t n_front,
                                                             const int32_t* __restrict__ f_st,
                                                             const uint64_t* __restrict__ f_out,
                                                             const uint64_t* __restrict__ f_end,
                                                             const uint32_t* __restrict__ f_unres,
                                                             int32_t* __restrict__ dec_st, uint64_t* __restrict__ out_len,
                                                             uint64_t* __restrict__ end_bit, uint32_t* __restrict__ unres) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_front) return;
  const uint32_t b = front[k];
  dec_st[b] = f_st[k];
  out_len[b] = f_out[k];
  end_bit[b] = f_end[k];
  unres[b] = f_unres[k];
}

// One workgroup per image whose chain stopped where no member starts (its last record's succ is kAskTail): the bytes
// from there to the image's end, 16 at a time -- all zero is a clean end (tape and block padding; gzip and Python's
// gzip accept it likewise), anything else is whatever the header checks say of that position.
__global__ __launch_bounds__(256) void zh_gzip_tail_kernel(const uint8_t* __restrict__ d_in,
                                                           const ZhZrImg* __restrict__ imgs,
                                                           const uint32_t* __restrict__ rec_ranges,
                                                           const uint32_t* __restrict__ list,
                                                           const uint64_t* __restrict__ mend, int32_t* succ) {
  __shared__ uint32_t s_nz;
  const uint32_t t = blockIdx.x, lo = rec_ranges[2 * t], hi = rec_ranges[2 * t + 1];
  if (hi == lo) return;
  const uint32_t node = list[hi - 1];
  if (succ[node] != kAskTail) return;  // (the same in every thread: nobody writes before the barrier below)
  const ZhZrImg g = imgs[t];
  const uint64_t a = g.up_off + mend[node], b = g.up_off + g.len;
  const uint64_t A = (a + 15) & ~(uint64_t)15, B = b & ~(uint64_t)15;
  uint32_t nz = 0;
  if (A >= B) {  // no whole chunk: at most 30 bytes
    if (a + threadIdx.x < b) nz = d_in[a + threadIdx.x];
  } else {
    if (a + threadIdx.x < A) nz = d_in[a + threadIdx.x];
    if (B + threadIdx.x < b) nz |= d_in[B + threadIdx.x];
    for (uint64_t c = A + 16ull * threadIdx.x; c < B; c += 16 * 256) {
      const Chunk16 x = *reinterpret_cast<const Chunk16*>(d_in + c);
      nz |= x.w[0] | x.w[1] | x.w[2] | x.w[3];
    }
  }
  if (threadIdx.x == 0) s_nz = 0;
  __syncthreads();
  if (nz) s_nz = 1u;  // (plain stores of the same value)
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t st = ZH_OK;
    if (s_nz) {
      st = quick_status(d_in + g.up_off, g.len, mend[node]);
      if (st == ZH_OK) st = ZH_ERR_INVALID_BUFFER;  // (cannot be: such a position is a hit)
    }
    succ[node] = st;
  }
}

// One thread per reached member, in walk order (r = its ordinal in the call, list[r] its node): its zh_gzip_member
// but for uoff, what the host needs beside it, and ulen[r] once more for the prefix sum.  A member that failed has
// no deflate bytes, no data and no trailer.  at[r]: its first byte in the upload.
__global__ __launch_bounds__(256) void zh_gzip_parse_kernel(const uint8_t* __restrict__ d_in,
                                                            const ZhZrImg* __restrict__ imgs, uint32_t n_img,
                                                            const uint64_t* __restrict__ hits,
                                                            const uint32_t* __restrict__ list,
                                                            const ZhGzipHead* __restrict__ heads,
                                                            const int32_t* __restrict__ dec_st,
                                                            const uint64_t* __restrict__ end_bit,
                                                            const uint64_t* __restrict__ out_len,
                                                            const int32_t* __restrict__ succ, uint32_t n_rec,
                                                            zh_gzip_member* __restrict__ mem, ZhGzipAux* __restrict__ aux,
                                                            uint64_t* __restrict__ ulen, uint64_t* __restrict__ at_up) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rec) return;
  const uint32_t node = list[r];
  const uint64_t at = hits[node];
  const ZhZrImg g = imgs[find_img(imgs, n_img, at)];
  const ZhGzipHead h = heads[node];
  const bool ok = h.status == ZH_OK && dec_st[node] == ZH_OK;
  zh_gzip_member m{};
  m.coff = at - g.up_off;
  m.cdata_off = m.coff + h.cdata_off;
  m.cdata_len = ok ? (end_bit[node] + 7) >> 3 : 0;
  m.ulen = ok ? out_len[node] : 0;
  if (ok && m.cdata_off + m.cdata_len + 8 <= g.len) {
    const uint8_t* __restrict__ tr = d_in + g.up_off + m.cdata_off + m.cdata_len;
    m.crc = ld32(tr);
    m.isize = ld32(tr + 4);
  }
  m.mtime = h.mtime;
  m.flg = (uint8_t)h.flg;
  m.xfl = (uint8_t)h.xfl;
  m.os = (uint8_t)h.os;
  m.extra_off = h.extra_off;
  m.extra_len = h.extra_len;
  m.name_off = h.name_off;
  m.name_len = h.name_len;
  m.comment_off = h.comment_off;
  m.comment_len = h.comment_len;
  mem[r] = m;
  ZhGzipAux x{};
  x.status = h.status != ZH_OK ? h.status : dec_st[node];
  x.succ_status = succ[node];
  x.hcrc_off = h.hcrc_off;
  aux[r] = x;
  ulen[r] = m.ulen;
  at_up[r] = at;
}

// out[i] = v[0] + .. + v[i - 1] for i in [0, n]: one workgroup, 256 values a step, 64 bits throughout (a member may
// hold more than 4 GiB)
__global__ __launch_bounds__(256) void zh_gzip_scan64_kernel(const uint64_t* __restrict__ v, uint32_t n,
                                                             uint64_t* __restrict__ out) {
  __shared__ uint64_t s[2][256];
  uint64_t carry = 0;
  for (uint32_t j = 0; j < n; j += 256) {
    const uint32_t i = j + threadIdx.x;
    const uint64_t x = i < n ? v[i] : 0u;
    uint32_t cur = 0;
    s[0][threadIdx.x] = x;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {  // (Hillis-Steele, two buffers)
      s[cur ^ 1][threadIdx.x] = s[cur][threadIdx.x] + (threadIdx.x >= d ? s[cur][threadIdx.x - d] : 0u);
      cur ^= 1;
      __syncthreads();
    }
    if (i < n) out[i] = carry + s[cur][threadIdx.x] - x;
    carry += s[cur][255];
    __syncthreads();  // (the next step writes s[0])
  }
  if (threadIdx.x == 0) out[n] = carry;
}

// a member's place in the uncompressed data of its image, from the sums over the call
__global__ __launch_bounds__(256) void zh_gzip_uoff_kernel(uint32_t n_img, const uint32_t* __restrict__ rec_ranges,
                                                           const uint64_t* __restrict__ sums, uint32_t n_rec,
                                                           zh_gzip_member* __restrict__ mem) {
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
  mem[r].uoff = sums[r] - sums[rec_ranges[2 * lo]];
}

// Every reached member's verdict, by the first of these that applies: its header's status; the decoder's (the sizing
// pass's, then the plan's -- out of room there reads ZH_ERR_SIZE); FHCRC, when present, against the low 16 bits of
// the CRC-32 of the header bytes before it; the CRC-32 of its data against the trailer's; its length mod 2^32 against
// ISIZE; what stands behind it.  pidx[r]: its stream in the plan, hidx[r]: its header among the FHCRC buffers.
__global__ __launch_bounds__(256) void zh_gzip_verify_kernel(const uint8_t* __restrict__ d_in,
                                                             const zh_gzip_member* __restrict__ mem,
                                                             const ZhGzipAux* __restrict__ aux,
                                                             const uint64_t* __restrict__ at_up,
                                                             const uint32_t* __restrict__ pidx,
                                                             const uint32_t* __restrict__ hidx, uint32_t n_rec,
                                                             const int32_t* __restrict__ plan_st,
                                                             const uint64_t* __restrict__ plan_len,
                                                             const uint32_t* __restrict__ plan_crc,
                                                             const uint32_t* __restrict__ head_crc,
                                                             int32_t* __restrict__ est) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rec) return;
  const zh_gzip_member m = mem[r];
  int32_t st = aux[r].status;
  if (st == ZH_OK && pidx[r] != kNone) {
    const uint32_t k = pidx[r];
    st = plan_st[k];
    if (st == ZH_ERR_DST_TOO_SMALL || (st == ZH_OK && plan_len[k] != m.ulen))
      st = ZH_ERR_SIZE;  // (the two decodes of one stream disagree: cannot be)
    else if (st == ZH_OK && hidx[r] != kNone && (head_crc[hidx[r]] & 0xffffu) != ld16(d_in + at_up[r] + aux[r].hcrc_off))
      st = ZH_ERR_CHECKSUM;
    else if (st == ZH_OK && plan_crc[k] != m.crc)
      st = ZH_ERR_CHECKSUM;
    else if (st == ZH_OK && (uint32_t)m.ulen != m.isize)
      st = ZH_ERR_SIZE;
  }
  if (st == ZH_OK) st = aux[r].succ_status;
  est[r] = st;
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
namespace {

// the bytes [0, to) of an arena back on the host in one copy (waits)
int fetch(zh_ctx* ctx, std::vector<uint8_t>& h, const Arena& ar, size_t to) {
  h.resize(to);
  if (!to) return ZH_OK;
  ZH_HIP(ctx, hipMemcpyAsync(h.data(), ar.base, to, hipMemcpyDeviceToHost, ctx->stream));
  ZH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ZH_OK;
}

// ZH_GZIP_SPEC_BYTES (a test aid): the sizing pass's budget; else 2 x the call's uploaded bytes + 64 MiB -- a real
// member is sized once, a false candidate usually dies within a few hundred bytes, and a crafted image cannot buy more
uint64_t spec_budget(uint64_t uploaded) {
  if (const char* e = getenv("ZH_GZIP_SPEC_BYTES")) return strtoull(e, nullptr, 10);
  return 2 * uploaded + (64ull << 20);
}

}  // namespace

extern "C" int zh_gzip_read_batch(zh_ctx* ctx, const void* const* images, const size_t* lens, size_t n, void** dsts,
                                  size_t* dst_lens, int32_t* statuses, zh_gzip_member** members, size_t* first) {
  if (!ctx || (n && (!images || !lens || !statuses)) || !dsts != !dst_lens || !members != !first) return ZH_ERR_ARGUMENT;
  if (dsts) clear_outputs(dsts, dst_lens, statuses, n);
  for (size_t t = 0; !dsts && t < n; t++) statuses[t] = ZH_OK;
  if (members) {
    *members = nullptr;
    for (size_t t = 0; t <= n; t++) first[t] = 0;
  }
  for (size_t t = 0; t < n; t++)
    if (!images[t] && lens[t]) return ZH_ERR_ARGUMENT;
  if (!n) return ZH_OK;
  Trace tr;
  int st;
  ScanUpload S;
  ScanHits H;
  if ((st = scan_upload(ctx, tr, "gzip", images, lens, n, 18, S))) return st;  // (no member is shorter than 18 bytes)
  if ((st = scan_hits<GzipSignature>(ctx, tr, "gzip", S, H))) return st;
  hipStream_t s = ctx->stream;
  const dim3 wg(256);
  const uint32_t n_img = S.n_img, n_hits = H.n_hits, N = n_hits + n_img;
  const uint8_t* const in = S.d_in.p;
  const ZhZrImg* const dimgs = S.imgs();
  const uint64_t* const hits = H.hits();

  // ---- the candidates' headers; the speculative sizing pass ----
  ZhGzipHead* heads;
  ZhBufDesc* bufs;
  ZhBufDesc* fbufs;
  int32_t *dec_st, *succ, *start, *f_st;
  uint32_t *body_pos, *unres, *hit_ranges, *n_front, *front_list, *f_unres;
  uint64_t *out_len, *end_bit, *mend, *f_out, *f_end;
  unsigned long long* used;
  Arena ex;
  ex.add(heads, n_hits);
  ex.add(bufs, n_hits);
  ex.add(dec_st, n_hits);
  ex.add(body_pos, n_hits);
  ex.add(out_len, n_hits);
  ex.add(end_bit, n_hits);
  ex.add(unres, n_hits);
  ex.add(front_list, n_hits);
  ex.add(fbufs, n_hits);
  ex.add(f_st, n_hits);
  ex.add(f_out, n_hits);
  ex.add(f_end, n_hits);
  ex.add(f_unres, n_hits);
  ex.add(succ, n_hits);
  ex.add(mend, n_hits);
  ex.add(hit_ranges, (size_t)n_img * 2);
  ex.add(start, n_img);
  ex.add(used, 1);
  ex.add(n_front, 1);
  Walk w;
  if ((st = scan_walk_alloc(ctx, S, H, ex, w))) return st;
  const dim3 node_grid((N + 255) / 256), img_grid((n_img + 255) / 256), hit_grid((n_hits + 255) / 256);
  ZH_HIP(ctx, hipMemsetAsync(ex.base, 0, ex.size, s));
  hipLaunchKernelGGL(zh_gzip_ranges_kernel, img_grid, wg, 0, s, in, dimgs, n_img, hits, n_hits, hit_ranges, start);
  const GzipBudget bd{used, spec_budget(S.up_total)};
  if (n_hits)
    hipLaunchKernelGGL(zh_gzip_head_kernel, dim3((n_hits + 3) / 4), wg, 0, s, in, dimgs, n_img, hits, n_hits, bd, heads,
                       bufs, dec_st, body_pos);
  tr.mark(ctx, "gzip: headers");
  ZhInflateArgs ia{};
  ia.bufs = bufs;
  ia.nbufs = n_hits;
  ia.data_format = ZH_DF_DEFLATE;
  ia.count_only = 1;
  ia.body_pos = body_pos;
  ia.out_len = out_len;
  ia.status = dec_st;
  ZhRecArgs spec{};
  spec.points = end_bit;
  spec.n = unres;
  spec.spec_used = used;
  spec.spec_budget = bd.budget;
  zh_launch_inflate_spec(s, in, ia, spec);
  ZH_HIP(ctx, hipGetLastError());
  unsigned long long h_used = 0;  // (what the speculative pass paid: read before a frontier round adds a real member's bytes)
  ZH_HIP(ctx, hipMemcpyAsync(&h_used, used, 8, hipMemcpyDeviceToHost, s));
  ZH_HIP(ctx, hipStreamSynchronize(s));
  tr.mark(ctx, "gzip: sizing pass");

  // ---- the walk; while a chain ends at a candidate the budget left unresolved, those are sized and it runs again ----
  uint32_t n_rec = 0;
  uint64_t rounds = 0;
  uint32_t *const j0 = w.j0, *const mark = w.mark;  // (plain pointers: a launch must not take the Walk along)
  const uint32_t *const ord = w.ord, *const list = w.list;
  for (;;) {
    hipLaunchKernelGGL(zh_gzip_next_kernel, node_grid, wg, 0, s, dimgs, n_img, hits, n_hits, (const uint32_t*)hit_ranges,
                       (const ZhGzipHead*)heads, (const int32_t*)dec_st, (const uint64_t*)end_bit, (const uint32_t*)unres,
                       N, j0, mark, succ, mend);
    walk_double(w, H.rounds, s);
    uint32_t front = 0;
    if (n_hits) {
      ZH_HIP(ctx, hipMemsetAsync(n_front, 0, 4, s));
      hipLaunchKernelGGL(zh_gzip_frontier_kernel, hit_grid, wg, 0, s, (const uint32_t*)mark, (const int32_t*)succ, n_hits,
                         front_list, n_front);
      ZH_HIP(ctx, hipGetLastError());
      ZH_HIP(ctx, hipMemcpyAsync(&front, n_front, 4, hipMemcpyDeviceToHost, s));
      ZH_HIP(ctx, hipStreamSynchronize(s));
    }
    if (!front) break;
    rounds++;
    hipLaunchKernelGGL(zh_gzip_front_head_kernel, dim3((front + 3) / 4), wg, 0, s, in, dimgs, n_img, hits,
                       (const uint32_t*)front_list, front, heads, bufs, fbufs, f_st, f_out, f_end, f_unres);
    ZhInflateArgs fa = ia;  // (body_pos: zero for every stream, whichever it is)
    fa.bufs = fbufs;
    fa.nbufs = front;
    fa.out_len = f_out;
    fa.status = f_st;
    ZhRecArgs fr = spec;
    fr.points = f_end;
    fr.n = f_unres;
    fr.spec_budget = ~0ull;
    zh_launch_inflate_spec(s, in, fa, fr);
    hipLaunchKernelGGL(zh_gzip_settle_kernel, dim3((front + 255) / 256), wg, 0, s, (const uint32_t*)front_list, front,
                       (const int32_t*)f_st, (const uint64_t*)f_out, (const uint64_t*)f_end, (const uint32_t*)f_unres, dec_st,
                       out_len, end_bit, unres);
  }
  walk_scan(w, s);
  if ((st = walk_count(ctx, w, &n_rec))) return st;
  ctx->gz_candidates = n_hits;
  ctx->gz_spec_bytes = h_used;
  ctx->gz_rounds = rounds;
  tr.mark(ctx, "gzip: reach + scan");

  // ---- the records ----
  zh_gzip_member* d_mem;
  ZhGzipAux* d_aux;
  uint32_t* d_rr;
  int32_t* d_start;
  uint64_t *d_ulen, *d_usum, *d_at;
  Arena out;
  out.add(d_mem, n_rec);
  out.add(d_aux, n_rec);
  out.add(d_rr, (size_t)n_img * 2);
  out.add(d_start, n_img);
  const size_t out_bytes = out.size;  // (what comes back: the arrays so far, in one copy)
  out.add(d_ulen, n_rec);
  out.add(d_usum, (size_t)n_rec + 1);
  out.add(d_at, n_rec);
  DevBuf d_rec;
  if (out.alloc(ctx, d_rec, 256) != hipSuccess) return ZH_ERR_NOMEM;
  out.bind();
  const dim3 rec_grid((n_rec + 255) / 256);
  hipLaunchKernelGGL(zh_walk_rec_ranges_kernel, img_grid, wg, 0, s, (const uint32_t*)hit_ranges, n_img, ord, d_rr);
  if (n_rec) {
    hipLaunchKernelGGL(zh_gzip_tail_kernel, dim3(n_img), wg, 0, s, in, dimgs, (const uint32_t*)d_rr, list,
                       (const uint64_t*)mend, succ);
    hipLaunchKernelGGL(zh_gzip_parse_kernel, rec_grid, wg, 0, s, in, dimgs, n_img, hits, list, (const ZhGzipHead*)heads,
                       (const int32_t*)dec_st, (const uint64_t*)end_bit, (const uint64_t*)out_len, (const int32_t*)succ,
                       n_rec, d_mem, d_aux, d_ulen, d_at);
  }
  hipLaunchKernelGGL(zh_gzip_scan64_kernel, dim3(1), wg, 0, s, (const uint64_t*)d_ulen, n_rec, d_usum);
  if (n_rec)
    hipLaunchKernelGGL(zh_gzip_uoff_kernel, rec_grid, wg, 0, s, n_img, (const uint32_t*)d_rr, (const uint64_t*)d_usum, n_rec,
                       d_mem);
  ZH_HIP(ctx, hipGetLastError());
  ZH_HIP(ctx, hipMemcpyAsync(d_start, start, (size_t)n_img * 4, hipMemcpyDeviceToDevice, s));
  std::vector<uint8_t> h_out;
  if ((st = fetch(ctx, h_out, out, out_bytes))) return st;
  const zh_gzip_member* const mem = out.host(h_out.data(), (const zh_gzip_member*)d_mem);
  const ZhGzipAux* const aux = out.host(h_out.data(), (const ZhGzipAux*)d_aux);
  const uint32_t* const rr = out.host(h_out.data(), (const uint32_t*)d_rr);
  const int32_t* const h_start = out.host(h_out.data(), (const int32_t*)d_start);
  tr.mark(ctx, "gzip: parse");

  // ---- the layout of the output: a member at the sum of the lengths before it; the FHCRC headers as buffers ----
  std::vector<uint64_t> aoff(n), alen(n, 0), p_soff, p_slen, p_doff, p_dcap;
  std::vector<uint32_t> pidx(n_rec, kNone), hidx(n_rec, kNone);
  std::vector<ZhBufDesc> hbufs;
  std::vector<ZhPieceDesc> hpieces;
  uint64_t out_total = 0;
  for (size_t t = 0; t < n; t++) {
    aoff[t] = out_total;
    for (uint32_t r = rr[2 * t]; r < rr[2 * t + 1]; r++) {
      const zh_gzip_member& m = mem[r];
      if (aux[r].status != ZH_OK) continue;
      pidx[r] = (uint32_t)p_soff.size();
      p_soff.push_back(S.up_off[t] + m.cdata_off);
      p_slen.push_back(m.cdata_len);
      p_doff.push_back(aoff[t] + m.uoff);
      p_dcap.push_back(m.ulen);
      alen[t] = m.uoff + m.ulen;
      if (aux[r].hcrc_off) {
        hidx[r] = (uint32_t)hbufs.size();
        ZhBufDesc hb{};
        hb.src_off = S.up_off[t] + m.coff;
        hb.src_len = aux[r].hcrc_off;
        hb.first_piece = (uint32_t)hpieces.size();
        for (uint64_t o = 0; o < hb.src_len; o += 32768)
          hpieces.push_back(ZhPieceDesc{hb.src_off + o, (uint32_t)std::min<uint64_t>(hb.src_len - o, 32768),
                                        (uint32_t)hbufs.size(), o});
        hb.npieces = (uint32_t)hpieces.size() - hb.first_piece;
        hbufs.push_back(hb);
      }
    }
    out_total = (out_total + alen[t] + 255) & ~(uint64_t)255;
    if (p_soff.size() > 0x7fffffffull || hpieces.size() > 0x7fffffffull) return ZH_ERR_ARGUMENT;
  }

  // ---- one decode, the headers' checksums, every verdict, the first failure of every image ----
  const uint32_t *d_pidx, *d_hidx;
  const ZhBufDesc* d_hbufs;
  const ZhPieceDesc* d_hpieces;
  int32_t* d_est;
  uint32_t *d_bad, *d_any, *d_pcrc, *d_padler, *d_plen, *d_hcrc, *d_hadler;
  Arena ar;
  ar.add(d_est, n_rec);
  ar.add(d_bad, n_img);
  const size_t ar_out = ar.size;  // (what comes back: the arrays so far, in one copy)
  ar.add(d_pidx, n_rec, pidx.data());
  ar.add(d_hidx, n_rec, hidx.data());
  ar.add(d_hbufs, hbufs.size(), hbufs.data());
  ar.add(d_hpieces, hpieces.size(), hpieces.data());
  ar.add(d_pcrc, hpieces.size());
  ar.add(d_padler, hpieces.size());
  ar.add(d_plen, hpieces.size());
  ar.add(d_hcrc, hbufs.size());
  ar.add(d_hadler, hbufs.size());
  ar.add(d_any, n_img);
  DevBuf d_ar, d_out;
  if (ar.alloc(ctx, d_ar, 256) != hipSuccess || dev_alloc(ctx, d_out, out_total + 256) != hipSuccess) return ZH_ERR_NOMEM;
  ar.bind();
  ZH_HIP(ctx, ar.upload(s));
  ZH_HIP(ctx, hipStreamSynchronize(s));  // (the tables are the scope's)
  PlanGuard pg;
  const size_t n_plan = p_soff.size();
  if (n_plan) {
    if ((st = zh_plan_uncompress(ctx, n_plan, p_soff.data(), p_slen.data(), p_doff.data(), p_dcap.data(), ZH_DF_DEFLATE, &pg.p)) ||
        (st = zh_plan_request_crc32(pg.p, 1)) || (st = zh_plan_run(pg.p, in, d_out.p)))
      return st;
  }
  if (!hbufs.empty()) {
    zh_launch_checksum_pieces(s, ctx->cktabs, in, d_hpieces, (uint32_t)hpieces.size(), nullptr, 1, 0, d_pcrc, d_padler, d_plen);
    zh_launch_checksum_combine(s, ctx->cktabs, d_hbufs, (uint32_t)hbufs.size(), d_pcrc, d_padler, d_plen, 1, 0, d_hcrc, d_hadler);
  }
  const int32_t* const plan_st = n_plan ? zh_plan_device_statuses(pg.p) : nullptr;
  const uint64_t* const plan_len = n_plan ? zh_plan_device_lens(pg.p) : nullptr;
  const uint32_t* const plan_crc = n_plan ? pg.p->buf_crc : nullptr;
  if (n_rec)
    hipLaunchKernelGGL(zh_gzip_verify_kernel, rec_grid, wg, 0, s, in, (const zh_gzip_member*)d_mem, (const ZhGzipAux*)d_aux,
                       (const uint64_t*)d_at, d_pidx, d_hidx, n_rec, plan_st, plan_len, plan_crc, (const uint32_t*)d_hcrc,
                       d_est);
  hipLaunchKernelGGL(zh_zip_reduce_kernel, dim3(n_img), wg, 0, s, (const uint32_t*)d_rr, (const int32_t*)d_est,
                     (const uint8_t*)nullptr, d_bad, d_any);
  ZH_HIP(ctx, hipGetLastError());
  std::vector<uint8_t> h_ar;
  if ((st = fetch(ctx, h_ar, ar, ar_out))) return st;
  const int32_t* const est = ar.host(h_ar.data(), (const int32_t*)d_est);
  const uint32_t* const bad = ar.host(h_ar.data(), (const uint32_t*)d_bad);
  tr.mark(ctx, "gzip: decode + verify");

  // ---- the results: data, statuses, the members of the images that are sound ----
  std::vector<int32_t> ist(n);
  size_t total = 0;
  for (size_t t = 0; t < n; t++) {
    ist[t] = h_start[t] != ZH_OK ? h_start[t] : bad[t] != kNone ? est[bad[t]] : (int32_t)ZH_OK;
    if (ist[t] == ZH_OK) total += rr[2 * t + 1] - rr[2 * t];
  }
  zh_gzip_member* e = nullptr;
  if (members) {
    e = (zh_gzip_member*)malloc((total ? total : 1) * sizeof(zh_gzip_member));
    if (!e) return ZH_ERR_NOMEM;
  }
  if (dsts) {
    if ((st = hand_out(ctx, d_out.p, aoff, alen, ist, dsts, dst_lens, statuses))) {
      free(e);
      return st;
    }
  } else {
    for (size_t t = 0; t < n; t++) statuses[t] = ist[t];
  }
  if (members) {
    size_t at = 0;
    for (size_t t = 0; t < n; t++) {
      first[t] = at;
      if (ist[t] != ZH_OK) continue;
      for (uint32_t r = rr[2 * t]; r < rr[2 * t + 1]; r++) e[at++] = mem[r];
    }
    first[n] = at;
    *members = e;
  }
  tr.mark(ctx, "gzip: download");
  return ZH_OK;
}

extern "C" int zh_debug_gzip_stats(zh_ctx* ctx, uint64_t* candidates, uint64_t* speculative_bytes, uint64_t* frontier_rounds) {
  if (!ctx) return ZH_ERR_ARGUMENT;
  if (candidates) *candidates = ctx->gz_candidates;
  if (speculative_bytes) *speculative_bytes = ctx->gz_spec_bytes;
  if (frontier_rounds) *frontier_rounds = ctx->gz_rounds;
  return ZH_OK;
}
