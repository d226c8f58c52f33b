// Seek indexes for foreign deflate streams (zh_seek_index_batch, zh_seek_read_ranges; the blob's layout and the point
// rule are include/zippy_hip.h's).
// Build: one upload, one uncompress plan over all streams whose tokens kernel records the chosen points as it goes
// (zh_inflate_tokens_kernel<.., kRec>, zh_inflate_split.hip; one workgroup a stream, never segment-wise), the points
// come down (16 bytes each), zh_seek_windows_kernel gathers every point's window out of the decoded output into the
// packed window store, the checksum pieces and combine kernels run with one "buffer" per interval, and the blobs are
// put together on the host from the points, the CRCs and the store.
// Read: range_geometry and RangeSpans (zh_range_host.h) with the point as the entry; the compressed spans and the
// windows of the touched intervals go up in one upload; every touched interval decodes on its own into a scratch
// slot [window | output] with zh_seek_inflate_kernel (the wave pair of zh_inflate_pair.h with a history length and
// a stop bit, ZhSeekStop), is checksummed there, and zh_range_clip_kernel puts its part into the range's slot; zh_seek_reduce_kernel settles the ranges.
#include "zh_gather.h"
#include "zh_range_host.h"
#include "zh_inflate_pair.h"

__global__ __launch_bounds__(128, 8) void zh_seek_inflate_kernel(const uint8_t* __restrict__ d_src,
                                                              uint8_t* __restrict__ d_dst,
                                                              ZhInflateArgs a, ZhSeekStop x) {
  zh_inflate_body<kFormSeek>(d_src, d_dst, a, x, ZhResume{});
}
// the intervals of a seek index (history lengths and stop bits beside a.start_bit)
extern "C" void zh_launch_seek_inflate(hipStream_t stream, const uint8_t* d_src, uint8_t* d_dst, ZhInflateArgs a,
                                       ZhSeekStop x) {
  if (!a.nbufs) return;
  hipLaunchKernelGGL(zh_seek_inflate_kernel, dim3(a.nbufs), dim3(128), 0, stream, d_src, d_dst, a, x);
}

// One workgroup a window: d_out[src, src + len) -> d_store[dst, dst + pad16(len)), dst a multiple of 16 of a buffer
// that is aligned itself: the source gathered at whatever alignment it has, aligned 16-byte stores, the last chunk's
// padding written as zeros.
__global__ __launch_bounds__(256) void zh_seek_windows_kernel(const uint8_t* __restrict__ d_out,
                                                              uint8_t* __restrict__ d_store,
                                                              const ZhClipDesc* __restrict__ wins) {
  const ZhClipDesc c = wins[blockIdx.x];
  uint8_t* d = d_store + c.dst;
  const uint32_t nv = c.len >> 4, rest = c.len & 15u;
  for (uint32_t j = threadIdx.x; j < nv; j += 256u)
    *reinterpret_cast<Chunk16*>(d + 16u * j) = gather16(d_out, c.src + 16ull * j);
  if (rest && threadIdx.x < 16u)
    d[16u * nv + threadIdx.x] = threadIdx.x < rest ? d_out[c.src + 16ull * nv + threadIdx.x] : (uint8_t)0;
}

// Device arrays of a range read.  Range r's intervals are first_iv[r] .. first_iv[r + 1] - 1, in index order.
struct ZhSeekReadArgs {
  const ZhBufDesc* bufs;       // [nintervals] dst_cap: window + promised bytes
  const uint64_t* iv_len;      // [nintervals] bytes the decoder left in out_len (the window's included)
  const int32_t* iv_status;    // [nintervals]
  const uint32_t* iv_crc;      // [nintervals] CRC-32 of what the slot holds behind the window
  const uint32_t* want_crc;    // [nintervals] the point's
  const uint32_t* first_iv;    // [nranges + 1]
  const int32_t* fixed_status; // [nranges] decided on the host (ZH_OK: by the intervals)
  const uint64_t* clip_len;    // [nranges]
  uint64_t* out_len;           // [nranges]
  int32_t* status;             // [nranges]
};

// One wave per range: its lowest interval that failed decides -- the decoder's status (ZH_ERR_DST_TOO_SMALL reads
// ZH_ERR_INVALID_BUFFER, as in zh_ranges_reduce_kernel), then the bytes made, then the CRC-32.
__global__ __launch_bounds__(64) void zh_seek_reduce_kernel(ZhSeekReadArgs a) {
  const uint32_t r = blockIdx.x;
  const unsigned lane = zh_lane();
  const int32_t fixed = a.fixed_status[r];
  if (fixed != ZH_OK) {
    if (lane == 0) {
      a.status[r] = fixed;
      a.out_len[r] = 0;
    }
    return;
  }
  auto verdict = [&](uint32_t k) -> int32_t {
    const int32_t st = a.iv_status[k];
    if (st != ZH_OK) return st == ZH_ERR_DST_TOO_SMALL ? (int32_t)ZH_ERR_INVALID_BUFFER : st;
    if (a.iv_len[k] != a.bufs[k].dst_cap) return ZH_ERR_INVALID_BUFFER;
    return a.iv_crc[k] != a.want_crc[k] ? (int32_t)ZH_ERR_CHECKSUM : (int32_t)ZH_OK;
  };
  const uint32_t b0 = a.first_iv[r], b1 = a.first_iv[r + 1];
  uint32_t bad = 0xffffffffu;
  for (uint32_t k = b0 + lane; k < b1; k += 64u)
    if (verdict(k) != ZH_OK && k < bad) bad = k;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bad = min(bad, (uint32_t)__shfl_xor(bad, o, 64));
  if (lane != 0) return;
  a.status[r] = bad == 0xffffffffu ? (int32_t)ZH_OK : verdict(bad);
  a.out_len[r] = bad == 0xffffffffu ? a.clip_len[r] : 0;
}

namespace {

inline uint64_t pad16(uint64_t v) { return (v + 15) & ~(uint64_t)15; }
inline uint64_t pad256(uint64_t v) { return (v + 255) & ~(uint64_t)255; }
inline uint64_t bytes_up_to(uint64_t bit) { return bit / 8 + ((bit & 7) != 0); }

int sync_stream(zh_ctx* ctx) {
  ZH_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ZH_OK;
}
// an arena's arrays allocated, cleared, uploaded and bound
int arena_up(zh_ctx* ctx, Arena& ar, DevBuf& mem) {
  ar.pad(256);
  if (ar.alloc(ctx, mem) != hipSuccess) {
    (void)hipGetLastError();
    ctx->last_error = "hipMalloc(seek arena)";
    return ZH_ERR_NOMEM;
  }
  ZH_HIP(ctx, hipMemsetAsync(ar.base, 0, ar.size, ctx->stream));
  ZH_HIP(ctx, ar.upload(ctx->stream));
  ar.bind();
  return ZH_OK;
}

// the checksum pieces of `len` bytes at d_data + off as buffer `buf`'s (whole pieces of 32 KiB and a last, shorter one)
void add_pieces(std::vector<ZhPieceDesc>& pieces, ZhBufDesc& b, uint32_t buf, uint64_t off, uint64_t len) {
  b.first_piece = (uint32_t)pieces.size();
  for (uint64_t o = 0; o < len; o += ZH_FRAG_SIZE)
    pieces.push_back(ZhPieceDesc{off + o, (uint32_t)std::min<uint64_t>(len - o, ZH_FRAG_SIZE), buf, o});
  b.npieces = (uint32_t)pieces.size() - b.first_piece;
}

// ---------------------------------------------------------------------------
// build
// ---------------------------------------------------------------------------
int host_format(const uint8_t* s, size_t len, int fmt) {  // zh_unwrap_kernel's detection (zippy.nim:108-125)
  if (fmt != ZH_DF_DETECT) return fmt;
  if (len > 18 && s[0] == 31 && s[1] == 139 && s[2] == 8 && (s[3] & 0xe0) == 0) return ZH_DF_GZIP;
  if (len > 6 && (s[0] & 0x0f) == 8 && (s[0] >> 4) <= 7 && (((unsigned)s[0] * 256u) + s[1]) % 31u == 0) return ZH_DF_ZLIB;
  return ZH_DF_DETECT;
}

// The streams `who` of a decode pass that ended well: their windows gathered, their intervals' CRC-32s made, their
// blobs put together.  pts: the pass's point lists (pairs), stream i's from pts_off[i] on, npts[i] of them.
int harvest(zh_ctx* ctx, const std::vector<size_t>& who, const uint8_t* d_out, const std::vector<uint64_t>& doff,
            const size_t* lens, const void* const* srcs, int data_format, uint64_t span, const std::vector<uint64_t>& pts,
            const std::vector<uint64_t>& pts_off, const std::vector<uint32_t>& npts, void** indexes, size_t* index_lens,
            int32_t* statuses) {
  if (who.empty()) return ZH_OK;
  hipStream_t s = ctx->stream;
  std::vector<std::vector<zh_seek_point>> lists(who.size());
  std::vector<uint64_t> store_off(who.size()), store_len(who.size()), first_iv(who.size());
  std::vector<ZhClipDesc> wins;
  std::vector<ZhBufDesc> ivs;
  std::vector<ZhPieceDesc> pieces;
  uint64_t store_total = 0;
  for (size_t w = 0; w < who.size(); w++) {
    const size_t i = who[w];
    const uint64_t* p = pts.data() + 2 * pts_off[i];
    std::vector<zh_seek_point>& L = lists[w];
    L.resize(npts[i]);
    store_off[w] = store_total;
    first_iv[w] = ivs.size();
    uint64_t woff = 0;
    for (uint32_t k = 0; k < npts[i]; k++) {
      const bool closing = k + 1 == npts[i];
      zh_seek_point& q = L[k];
      q.bit_off = p[2 * k];
      q.out_off = p[2 * k + 1];
      q.win_off = woff;
      q.win_len = closing ? 0u : (uint32_t)std::min<uint64_t>(q.out_off, ZH_SEEK_WINDOW);
      q.crc32 = 0;
      if (q.win_len) {
        if (wins.size() >= 0x7fffffffull) return ZH_ERR_ARGUMENT;
        wins.push_back(ZhClipDesc{doff[i] + q.out_off - q.win_len, store_total + woff, q.win_len, 0});
      }
      woff += pad16(q.win_len);
      if (!closing) {
        ZhBufDesc b;
        memset(&b, 0, sizeof(b));
        if (pieces.size() + (p[2 * k + 3] - q.out_off) / ZH_FRAG_SIZE + 1 > 0x7fffffffull) return ZH_ERR_ARGUMENT;
        add_pieces(pieces, b, (uint32_t)ivs.size(), doff[i] + q.out_off, p[2 * k + 3] - q.out_off);
        ivs.push_back(b);
      }
    }
    store_len[w] = woff;
    store_total += pad256(woff);
  }
  if (ivs.size() > 0x7fffffffull) return ZH_ERR_ARGUMENT;
  ZhClipDesc* d_wins = nullptr;
  ZhBufDesc* d_ivs = nullptr;
  ZhPieceDesc* d_pieces = nullptr;
  uint32_t *piece_crc = nullptr, *piece_len = nullptr, *iv_crc = nullptr;
  uint8_t* d_store = nullptr;
  Arena ar;
  DevBuf mem;
  ar.add(d_wins, wins.size(), wins.data());
  ar.add(d_ivs, ivs.size(), ivs.data());
  ar.add(d_pieces, pieces.size(), pieces.data());
  ar.add(piece_crc, pieces.size());
  ar.add(piece_len, pieces.size());
  ar.add(iv_crc, ivs.size());
  ar.add(d_store, store_total);
  if (const int st = arena_up(ctx, ar, mem)) return st;
  if (!wins.empty())
    hipLaunchKernelGGL(zh_seek_windows_kernel, dim3((uint32_t)wins.size()), dim3(256), 0, s, d_out, d_store, d_wins);
  zh_launch_checksum_pieces(s, ctx->cktabs, d_out, d_pieces, (uint32_t)pieces.size(), nullptr, 1, 0, piece_crc, nullptr,
                            piece_len);
  if (!ivs.empty())
    zh_launch_checksum_combine(s, ctx->cktabs, d_ivs, (uint32_t)ivs.size(), piece_crc, nullptr, piece_len, 1, 0, iv_crc,
                               nullptr);
  ZH_HIP(ctx, hipGetLastError());
  std::vector<uint32_t> crcs(ivs.size());
  std::vector<uint8_t> store(store_total);
  if (!crcs.empty()) ZH_HIP(ctx, hipMemcpyAsync(crcs.data(), iv_crc, crcs.size() * 4, hipMemcpyDeviceToHost, s));
  if (store_total) ZH_HIP(ctx, hipMemcpyAsync(store.data(), d_store, store_total, hipMemcpyDeviceToHost, s));
  if (const int st = sync_stream(ctx)) return st;
  for (size_t w = 0; w < who.size(); w++) {
    const size_t i = who[w];
    std::vector<zh_seek_point>& L = lists[w];
    for (size_t k = 0; k + 1 < L.size(); k++) L[k].crc32 = crcs[first_iv[w] + k];
    zh_seek_header h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, ZH_SEEK_MAGIC, 8);
    h.version = ZH_SEEK_VERSION;
    h.data_format = (uint32_t)host_format((const uint8_t*)srcs[i], lens[i], data_format);
    h.src_len = lens[i];
    h.total = L.back().out_off;
    h.span = span;
    h.n_points = L.size();
    h.window_bytes = store_len[w];
    const size_t blob_len = sizeof(h) + L.size() * sizeof(zh_seek_point) + (size_t)store_len[w];
    uint8_t* blob = (uint8_t*)malloc(blob_len);
    if (!blob) {
      statuses[i] = ZH_ERR_NOMEM;
      continue;
    }
    memcpy(blob, &h, sizeof(h));
    memcpy(blob + sizeof(h), L.data(), L.size() * sizeof(zh_seek_point));
    if (store_len[w]) memcpy(blob + sizeof(h) + L.size() * sizeof(zh_seek_point), store.data() + store_off[w], store_len[w]);
    indexes[i] = blob;
    index_lens[i] = blob_len;
  }
  return ZH_OK;
}

}  // namespace

static_assert(sizeof(zh_seek_header) == 64 && sizeof(zh_seek_point) == 32, "the blob's layout is the header's");

// The passes are zh_uncompress_batch's (zh_host_batch.hip): gzip members decode into ISIZE bytes, zlib and raw
// streams into a guess; what outgrows its room is sized (a count-only pass) or given the expansion bound, and decoded
// once more.  A stream's points are those of the pass that settled it.
extern "C" int zh_seek_index_batch(zh_ctx* ctx, const void* const* srcs, const size_t* lens, size_t n, int data_format,
                                   uint64_t span, void** indexes, size_t* index_lens, void** dsts, size_t* dst_lens,
                                   int32_t* statuses) {
  if (!ctx || (n && (!srcs || !lens || !indexes || !index_lens || !statuses)) || (!dsts != !dst_lens)) return ZH_ERR_ARGUMENT;
  clear_outputs(indexes, index_lens, statuses, n);
  if (dsts)
    for (size_t i = 0; i < n; i++) {
      dsts[i] = nullptr;
      dst_lens[i] = 0;
    }
  if (span == 0) span = ZH_SEEK_DEFAULT_SPAN;
  if (span < ZH_SEEK_WINDOW) return ZH_ERR_ARGUMENT;
  if (data_format < ZH_DF_DETECT || data_format > ZH_DF_DEFLATE) {
    for (size_t i = 0; i < n; i++) statuses[i] = ZH_ERR_INVALID_FORMAT;
    return ZH_ERR_INVALID_FORMAT;
  }
  for (size_t i = 0; i < n; i++)
    if (!srcs[i] && lens[i]) return ZH_ERR_ARGUMENT;
  if (!n) return ZH_OK;
  if (n > 0x7fffffffull) return ZH_ERR_ARGUMENT;
  ZH_HIP(ctx, hipSetDevice(ctx->device));
  Trace tr;
  int st;
  std::vector<uint64_t> cap(n, 0);
  std::vector<char> guessed(n, 0), active(n, 1);
  for (size_t i = 0; i < n; i++) {
    const uint8_t* s8 = (const uint8_t*)srcs[i];
    const int f = host_format(s8, lens[i], data_format);
    const uint64_t max_out = (uint64_t)lens[i] * 1032 + 64;  // deflate cannot expand further
    if (f == ZH_DF_GZIP && lens[i] >= 18) {
      const uint8_t* t = s8 + lens[i] - 4;
      cap[i] = std::min<uint64_t>(t[0] | (t[1] << 8) | (t[2] << 16) | ((uint64_t)t[3] << 24), max_out);
    } else if (f == ZH_DF_ZLIB || f == ZH_DF_DEFLATE) {
      guessed[i] = 1;
      cap[i] = std::min<uint64_t>((uint64_t)lens[i] * 4 + 65536, max_out);
    }
  }
  DevBuf d_src;
  std::vector<uint64_t> soff, slen;
  if ((st = zhh_upload(ctx, srcs, lens, n, d_src, soff, slen))) return st;
  tr.mark(ctx, "seek index: upload");
  // Room for the point lists: a stream expands at most 1032 : 1, so the rule chooses at most (1032 * len + 64) / span
  // points behind the first, and the closing entry.  Where all the lists together would take more than kListBytes,
  // every list gets 4096 entries; the kernel counts what it could not write, and such a pass runs once more with
  // the counts as the lists' sizes (ZH_SEEK_FIRST_CAP, a test aid: the first attempt's entries a list).
  constexpr uint64_t kListBytes = 256ull << 20;
  const char* first_cap_env = getenv("ZH_SEEK_FIRST_CAP");
  std::vector<uint64_t> want_pts(n, 0);  // (0: the bound)
  int pass = 1;
  for (int turn = 0; turn < 6; turn++) {
    std::vector<uint64_t> doff(n), dcap(n), slen_now(n);
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) {
      const bool runs = active[i] && (pass != 0 || guessed[i]);
      slen_now[i] = runs ? slen[i] : 0;
      dcap[i] = pass == 0 || !runs ? 0 : cap[i];
      doff[i] = total;
      total += pad256(dcap[i]);
    }
    DevBuf d_dst;
    if (dev_alloc(ctx, d_dst, total + 256) != hipSuccess) return ZH_ERR_NOMEM;
    PlanGuard pg;
    if ((st = zh_plan_uncompress(ctx, n, soff.data(), slen_now.data(), doff.data(), dcap.data(), data_format, &pg.p))) return st;
    pg.p->segmented = false;  // one workgroup a stream: the segment-wise decoders record nothing
    plan_set_count_only(pg.p, pass == 0);
    std::vector<uint64_t> pts_off(n);
    std::vector<uint32_t> pts_cap(n), npts(n, 0);
    std::vector<uint64_t> pts;
    Arena ar;
    DevBuf rec_mem;
    ZhRecArgs& rec = pg.p->rec;
    if (pass != 0) {
      uint64_t sum = 0;
      for (int round = 0; round < 2; round++) {
        sum = 0;
        for (size_t i = 0; i < n; i++) {
          uint64_t c = slen_now[i] ? (1032 * slen_now[i] + 64) / span + 2 : 0;
          if (want_pts[i]) c = want_pts[i];
          else if (round == 1) c = std::min<uint64_t>(c, 4096);
          else if (first_cap_env && slen_now[i]) c = std::min<uint64_t>(c, std::max(1, atoi(first_cap_env)));
          pts_cap[i] = (uint32_t)std::min<uint64_t>(c, 0x7fffffffu);
          pts_off[i] = sum;
          sum += pts_cap[i];
        }
        if (sum * 16 <= kListBytes) break;
      }
      const uint64_t* c_off = nullptr;
      const uint32_t* c_cap = nullptr;
      ar.add(rec.points, (size_t)sum * 2);
      ar.add(c_off, n, pts_off.data());
      ar.add(c_cap, n, pts_cap.data());
      ar.add(rec.n, n);
      if ((st = arena_up(ctx, ar, rec_mem))) return st;
      rec.off = c_off;
      rec.cap = c_cap;
      rec.span = span;
    }
    tr.mark(ctx, "seek index: alloc + plan");
    if ((st = zh_plan_run(pg.p, d_src.p, d_dst.p))) return st;
    std::vector<uint64_t> olen(n);
    std::vector<int32_t> ost(n);
    if ((st = zh_plan_results(pg.p, olen.data(), ost.data()))) return st;
    tr.mark(ctx, "seek index: decode");
    if (pass == 0) {
      for (size_t i = 0; i < n; i++)
        if (active[i] && guessed[i]) cap[i] = olen[i];
      pass = 2;
      continue;
    }
    ZH_HIP(ctx, hipMemcpyAsync(npts.data(), rec.n, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if ((st = sync_stream(ctx))) return st;
    bool short_list = false;
    for (size_t i = 0; i < n; i++)
      if (active[i] && ost[i] == ZH_OK && npts[i] > pts_cap[i]) {
        want_pts[i] = npts[i];
        short_list = true;
      }
    if (short_list) {  // a list was cut short: the same pass once more, with room for what was counted
      if (getenv("ZH_TRACE")) fprintf(stderr, "zippy_hip: seek index: point lists cut short, decoding once more\n");
      continue;
    }
    pts.resize((size_t)(pts_off[n - 1] + pts_cap[n - 1]) * 2);
    if (!pts.empty()) ZH_HIP(ctx, hipMemcpyAsync(pts.data(), rec.points, pts.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    if ((st = sync_stream(ctx))) return st;
    bool again = false, size_first = false;
    std::vector<char> take(n, 0);
    std::vector<size_t> who;
    for (size_t i = 0; i < n; i++) {
      if (!active[i]) continue;
      statuses[i] = ost[i];
      if (ost[i] == ZH_ERR_DST_TOO_SMALL && pass == 1) {
        if (guessed[i])
          size_first = true;
        else
          cap[i] = (uint64_t)lens[i] * 1032 + 64;
        again = true;
        continue;
      }
      active[i] = 0;
      if (ost[i] == ZH_ERR_DST_TOO_SMALL) statuses[i] = ZH_ERR_CHECKSUM;  // (as zh_uncompress_batch reads it)
      if (ost[i] != ZH_OK) continue;
      if (npts[i] < 2) {  // (a decoder that recorded nothing took this stream: no index can be made)
        ctx->last_error = "seek index: no points recorded";
        return ZH_ERR_DEVICE;
      }
      take[i] = 1;
      who.push_back(i);
    }
    if ((st = harvest(ctx, who, d_dst.p, doff, lens, srcs, data_format, span, pts, pts_off, npts, indexes, index_lens,
                      statuses)))
      return st;
    tr.mark(ctx, "seek index: windows + crcs");
    if (dsts) {
      for (size_t i = 0; i < n; i++)
        if (take[i] && statuses[i] != ZH_OK) take[i] = 0;
      if ((st = zhh_download(ctx, d_dst.p, n, doff, olen, take, dsts, dst_lens, statuses))) return st;
      for (size_t i = 0; i < n; i++)
        if (take[i] && statuses[i] != ZH_OK && indexes[i]) {  // (no data, no index)
          free(indexes[i]);
          indexes[i] = nullptr;
          index_lens[i] = 0;
        }
      tr.mark(ctx, "seek index: download");
    }
    if (!again || pass == 2) break;
    pass = size_first ? 0 : 2;
  }
  return ZH_OK;
}

// ---------------------------------------------------------------------------
// read
// ---------------------------------------------------------------------------
namespace {

// what can be said of a blob's point list without decoding (include/zippy_hip.h)
bool points_sound(const zh_seek_point* e, size_t n, uint64_t src_len, uint64_t total, uint64_t window_bytes) {
  if (n < 2 || n > 0xfffffffeull || e[0].out_off != 0 || e[n - 1].out_off != total) return false;
  for (size_t k = 0; k < n; k++) {
    const bool closing = k + 1 == n;
    if (closing ? bytes_up_to(e[k].bit_off) > src_len : e[k].bit_off / 8 >= src_len) return false;
    if (e[k].win_len != (closing ? 0u : (uint32_t)std::min<uint64_t>(e[k].out_off, ZH_SEEK_WINDOW))) return false;
    if ((e[k].win_off & 15u) || e[k].win_off > window_bytes || pad16(e[k].win_len) > window_bytes - e[k].win_off) return false;
    if (closing) break;
    if (e[k + 1].bit_off <= e[k].bit_off || e[k + 1].out_off < e[k].out_off) return false;
    const uint64_t bytes = bytes_up_to(e[k + 1].bit_off) - e[k].bit_off / 8;
    if (bytes <= (~0ull - 64) / 1032 && e[k + 1].out_off - e[k].out_off > bytes * 1032 + 64) return false;
  }
  return true;
}

}  // namespace

extern "C" int zh_seek_read_ranges(zh_ctx* ctx, const void* const* srcs, const size_t* lens, size_t n_streams,
                                   const void* const* indexes, const size_t* index_lens, size_t n_ranges,
                                   const uint64_t* range_stream, const uint64_t* range_off, const uint64_t* range_len,
                                   void** dsts, size_t* dst_lens, int32_t* statuses) {
  if (!ctx || (n_streams && (!srcs || !lens || !indexes || !index_lens)) || (n_ranges && (!dsts || !dst_lens || !statuses)))
    return ZH_ERR_ARGUMENT;
  clear_outputs(dsts, dst_lens, statuses, n_ranges);
  for (size_t s = 0; s < n_streams; s++)
    if ((!srcs[s] && lens[s]) || (!indexes[s] && index_lens[s])) return ZH_ERR_ARGUMENT;
  if (n_ranges > 0x7fffffffull) return ZH_ERR_ARGUMENT;
  // the blobs' headers and point lists (copied: a blob lies at whatever alignment the caller keeps it); a blob whose
  // header cannot be right has no list, which range_geometry's verdict reads as unsound
  std::vector<zh_seek_point> pts;
  std::vector<size_t> first(n_streams + 1, 0);
  std::vector<zh_seek_header> hdr(n_streams);
  std::vector<const void*> up_src(2 * n_streams, nullptr);  // owner 2 s: the stream's bytes, 2 s + 1: its window store
  for (size_t s = 0; s < n_streams; s++) {
    first[s] = pts.size();
    zh_seek_header& h = hdr[s];
    memset(&h, 0, sizeof(h));
    const size_t len = index_lens[s];
    if (len < sizeof(h)) continue;
    memcpy(&h, indexes[s], sizeof(h));
    const uint64_t room = len - sizeof(h);
    const bool ok = memcmp(h.magic, ZH_SEEK_MAGIC, 8) == 0 && h.version == ZH_SEEK_VERSION && h.src_len == lens[s] &&
                    h.n_points <= room / sizeof(zh_seek_point) && h.window_bytes == room - h.n_points * sizeof(zh_seek_point);
    if (!ok) {
      memset(&h, 0, sizeof(h));
      continue;
    }
    pts.resize(first[s] + (size_t)h.n_points);
    if (h.n_points) memcpy(pts.data() + first[s], (const uint8_t*)indexes[s] + sizeof(h), (size_t)h.n_points * sizeof(zh_seek_point));
    up_src[2 * s] = srcs[s];
    up_src[2 * s + 1] = (const uint8_t*)indexes[s] + sizeof(h) + (size_t)h.n_points * sizeof(zh_seek_point);
  }
  first[n_streams] = pts.size();
  std::vector<RangeGeo> geo;
  if (const int st = range_geometry(
          n_streams, pts.data(), first.data(), n_ranges, range_stream, range_off, range_len,
          [&](size_t s, const zh_seek_point* e, size_t ne) {
            return ne != 0 && points_sound(e, ne, lens[s], hdr[s].total, hdr[s].window_bytes);
          },
          [](const zh_seek_point& x) { return x.out_off; }, geo))
    return st;
  if (!n_ranges) return ZH_OK;
  Trace tr;
  // the upload: the compressed spans and the windows of the touched intervals, merged owner by owner
  RangeSpans up;
  for (size_t r = 0; r < n_ranges; r++) {
    const RangeGeo& q = geo[r];
    if (q.fixed != ZH_OK || q.k0 > q.k1) continue;
    const size_t s = (size_t)range_stream[r];
    const zh_seek_point* e = pts.data() + first[s];
    up.add(2 * s, e[q.k0].bit_off / 8, std::min<uint64_t>(bytes_up_to(e[q.k1 + 1].bit_off), lens[s]));
    for (size_t k = q.k0; k <= q.k1; k++)
      if (e[k].win_len && e[k + 1].out_off > e[k].out_off) up.add(2 * s + 1, e[k].win_off, e[k].win_off + pad16(e[k].win_len));
  }
  up.place(up_src.data());
  const uint64_t up_total = up.up_total;
  ZH_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf d_src;
  if (dev_alloc(ctx, d_src, up_total + 256) != hipSuccess) return ZH_ERR_NOMEM;
  if (const int st = zhh_upload_slices(ctx, up.sp.data(), up.soff, up.slen, up_total, d_src.p)) return st;
  tr.mark(ctx, "seek ranges: upload");
  // the intervals, range by range; groups of ranges whose scratch slots fit the budget take turns
  struct Group {
    uint32_t iv0, niv, wclip0, nwclip, clip0, nclip, piece0, npiece;
  };
  const uint64_t budget = scratch_budget();
  std::vector<ZhBufDesc> ivs;
  std::vector<uint64_t> start_bit, stop_bit, doff(n_ranges), clip_len(n_ranges);
  std::vector<uint32_t> hist, want_crc, first_iv(n_ranges + 1);
  std::vector<int32_t> fixed(n_ranges);
  std::vector<ZhClipDesc> wclips, clips;
  std::vector<ZhPieceDesc> pieces;
  std::vector<Group> groups;
  Group g{0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t gbytes = 0, gmax = 0, dst_total = 0;
  bool gany = false;
  for (size_t r = 0; r < n_ranges; r++) {
    const RangeGeo& q = geo[r];
    fixed[r] = q.fixed;
    clip_len[r] = q.end - q.off;
    doff[r] = dst_total;
    dst_total += pad256(clip_len[r]);
    first_iv[r] = (uint32_t)ivs.size();
    if (q.fixed != ZH_OK || q.k0 > q.k1) continue;
    const size_t si = (size_t)range_stream[r];
    const zh_seek_point* e = pts.data() + first[si];
    auto slot_bytes = [&](size_t k) { return pad256(e[k].win_len + (e[k + 1].out_off - e[k].out_off) + kGatherSlack); };
    uint64_t need = 0;
    for (size_t k = q.k0; k <= q.k1; k++) need += slot_bytes(k);
    if (gany && gbytes + need > budget) {
      groups.push_back(g);
      gmax = std::max(gmax, gbytes);
      g = Group{(uint32_t)ivs.size(), 0, (uint32_t)wclips.size(), 0, (uint32_t)clips.size(), 0, (uint32_t)pieces.size(), 0};
      gbytes = 0;
    }
    gany = true;
    if (ivs.size() + (q.k1 - q.k0 + 1) > 0x7fffffffull) return ZH_ERR_ARGUMENT;
    const RangeSpans::Span& x = up.holding(2 * si, e[q.k0].bit_off / 8);
    for (size_t k = q.k0; k <= q.k1; k++) {
      const uint64_t bs = e[k].out_off, be = e[k + 1].out_off;
      if (be == bs) continue;  // (an empty interval: nothing of it lies in any range)
      const uint32_t wl = e[k].win_len;
      ZhBufDesc b = block_decoder_desc(x.dev, x.hi - x.lo, gbytes, wl + (be - bs));
      if (pieces.size() + (be - bs) / ZH_FRAG_SIZE + 1 > 0x7fffffffull) return ZH_ERR_ARGUMENT;
      add_pieces(pieces, b, (uint32_t)ivs.size(), gbytes + wl, be - bs);
      ivs.push_back(b);
      start_bit.push_back(e[k].bit_off - 8 * x.lo);
      stop_bit.push_back(e[k + 1].bit_off - 8 * x.lo);
      hist.push_back(wl);
      want_crc.push_back(e[k].crc32);
      if (wl) {
        const RangeSpans::Span& w = up.holding(2 * si + 1, e[k].win_off);
        append_clips(wclips, w.dev + (e[k].win_off - w.lo), gbytes, wl);
      }
      const uint64_t lo = std::max(q.off, bs), hi = std::min(q.end, be);
      append_clips(clips, gbytes + wl + (lo - bs), doff[r] + (lo - q.off), hi - lo);
      gbytes += slot_bytes(k);
    }
    if (clips.size() > 0x7fffffffull || wclips.size() > 0x7fffffffull) return ZH_ERR_ARGUMENT;
    g.niv = (uint32_t)ivs.size() - g.iv0;
    g.nwclip = (uint32_t)wclips.size() - g.wclip0;
    g.nclip = (uint32_t)clips.size() - g.clip0;
    g.npiece = (uint32_t)pieces.size() - g.piece0;
  }
  first_iv[n_ranges] = (uint32_t)ivs.size();
  if (gany) {
    groups.push_back(g);
    gmax = std::max(gmax, gbytes);
  }
  if (groups.size() > 1 && getenv("ZH_TRACE"))
    fprintf(stderr, "zippy_hip: seek scratch for %zu groups of ranges (%zu ranges)\n", groups.size(), n_ranges);
  const size_t niv = ivs.size();
  ZhSeekReadArgs a{};
  ZhBufDesc* d_ivs = nullptr;
  uint64_t *d_start = nullptr, *d_stop = nullptr, *iv_len = nullptr;
  uint32_t *d_hist = nullptr, *piece_crc = nullptr, *piece_len = nullptr, *iv_crc = nullptr;
  int32_t* iv_status = nullptr;
  ZhClipDesc *d_wclips = nullptr, *d_clips = nullptr;
  ZhPieceDesc* d_pieces = nullptr;
  Arena ar;
  DevBuf mem, d_dst, scratch;
  ar.add(d_ivs, niv, ivs.data());
  ar.add(d_start, niv, start_bit.data());
  ar.add(d_stop, niv, stop_bit.data());
  ar.add(d_hist, niv, hist.data());
  ar.add(a.want_crc, niv, want_crc.data());
  ar.add(iv_len, niv);
  ar.add(iv_status, niv);
  ar.add(iv_crc, niv);
  ar.add(d_wclips, wclips.size(), wclips.data());
  ar.add(d_clips, clips.size(), clips.data());
  ar.add(d_pieces, pieces.size(), pieces.data());
  ar.add(piece_crc, pieces.size());
  ar.add(piece_len, pieces.size());
  ar.add(a.first_iv, n_ranges + 1, first_iv.data());
  ar.add(a.fixed_status, n_ranges, fixed.data());
  ar.add(a.clip_len, n_ranges, clip_len.data());
  ar.add(a.out_len, n_ranges);
  ar.add(a.status, n_ranges);
  if (const int st = arena_up(ctx, ar, mem)) return st;
  if (dev_alloc(ctx, d_dst, dst_total + 256) != hipSuccess || (gmax && dev_alloc(ctx, scratch, gmax + 256) != hipSuccess)) {
    (void)hipGetLastError();
    return ZH_ERR_NOMEM;
  }
  a.bufs = d_ivs;
  a.iv_len = iv_len;
  a.iv_status = iv_status;
  a.iv_crc = iv_crc;
  for (const Group& q : groups) {
    zh_launch_range_clip(s, d_src.p, scratch.p, d_wclips + q.wclip0, q.nwclip);
    ZhInflateArgs ia = block_decoder_args(d_ivs + q.iv0, d_start + q.iv0, q.niv, iv_len + q.iv0, iv_status + q.iv0);
    ia.single_block = 0;
    zh_launch_seek_inflate(s, d_src.p, scratch.p, ia, ZhSeekStop{d_hist + q.iv0, d_stop + q.iv0});
    zh_launch_checksum_pieces(s, ctx->cktabs, scratch.p, d_pieces + q.piece0, q.npiece, nullptr, 1, 0, piece_crc + q.piece0,
                              nullptr, piece_len + q.piece0);
    zh_launch_range_clip(s, scratch.p, d_dst.p, d_clips + q.clip0, q.nclip);
    ZH_HIP(ctx, hipGetLastError());
  }
  if (niv) zh_launch_checksum_combine(s, ctx->cktabs, d_ivs, (uint32_t)niv, piece_crc, nullptr, piece_len, 1, 0, iv_crc, nullptr);
  hipLaunchKernelGGL(zh_seek_reduce_kernel, dim3((uint32_t)n_ranges), dim3(64), 0, s, a);
  ZH_HIP(ctx, hipGetLastError());
  std::vector<uint64_t> olen(n_ranges);
  std::vector<int32_t> ost(n_ranges);
  ZH_HIP(ctx, hipMemcpyAsync(olen.data(), a.out_len, n_ranges * 8, hipMemcpyDeviceToHost, s));
  ZH_HIP(ctx, hipMemcpyAsync(ost.data(), a.status, n_ranges * 4, hipMemcpyDeviceToHost, s));
  if (const int st = sync_stream(ctx)) return st;
  ctx->rg_uploaded = up_total;
  ctx->rg_in_place = 0;
  ctx->rg_via_scratch = niv;
  tr.mark(ctx, "seek ranges: decode");
  if (const int st = hand_out(ctx, d_dst.p, doff, olen, ost, dsts, dst_lens, statuses)) return st;
  tr.mark(ctx, "seek ranges: download");
  return ZH_OK;
}
