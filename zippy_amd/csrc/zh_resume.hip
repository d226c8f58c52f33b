// Resumable uncompress (zh_uncompress_resume_batch; the state's layout and the contract are include/zippy_hip.h's):
// streams decoded as their bytes arrive, whole deflate blocks at a time.
// The container's header and trailer, the states and the running checksum are the host's; every live stream's bytes
// and window go up in one upload; groups of streams whose scratch slots [window | max_out | spare] (the window ends at
// a multiple of 16) fit the budget
// take turns: zh_range_clip_kernel puts the windows in front of the slots, zh_resume_inflate_kernel -- the wave pair
// of zh_inflate_pair.h in its third form, which runs until the input or the slot gives out and reports the last block
// boundary it got through -- decodes, the checksum pieces and combine kernels run over the delivered bytes with one
// "buffer" per stream, and one download a group brings results and data down.  The new window is the tail of
// [old window | delivered], both of which the host holds by then.
#include "zh_gather.h"
#include "zh_range_host.h"
#include "zh_inflate_pair.h"

__global__ __launch_bounds__(128, 8) void zh_resume_inflate_kernel(const uint8_t* __restrict__ d_src,
                                                                uint8_t* __restrict__ d_dst,
                                                                ZhInflateArgs a, ZhResume r) {
  zh_inflate_body<kFormResume>(d_src, d_dst, a, ZhSeekStop{}, r);
}
// streams that resume (history lengths, `last` flags, boundaries and reasons beside a.start_bit)
extern "C" void zh_launch_resume_inflate(hipStream_t stream, const uint8_t* d_src, uint8_t* d_dst, ZhInflateArgs a,
                                         ZhResume r) {
  if (!a.nbufs) return;
  hipLaunchKernelGGL(zh_resume_inflate_kernel, dim3(a.nbufs), dim3(128), 0, stream, d_src, d_dst, a, r);
}

namespace {

inline uint64_t pad16(uint64_t v) { return (v + 15) & ~(uint64_t)15; }
inline uint64_t pad256(uint64_t v) { return (v + 255) & ~(uint64_t)255; }

// ---- the running checksum: crc(A || B) and adler(A || B) from those of A and B and B's length ----
constexpr uint32_t kCrcPoly = 0xedb88320u;
uint32_t crc_mul(uint32_t a, uint32_t b) {  // a(x) * b(x) mod P, reflected (x^0: bit 31)
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    if (a & 0x80000000u) p ^= b;
    a <<= 1;
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}
uint32_t crc32_join(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
  uint32_t x = 0x80000000u, sq = 0x00800000u;  // x^0, x^8: x = x^(8 len_b)
  for (uint64_t n = len_b; n; n >>= 1) {
    if (n & 1) x = crc_mul(sq, x);
    sq = crc_mul(sq, sq);
  }
  return crc_mul(x, crc_a) ^ crc_b;
}
uint32_t adler32_join(uint32_t ad_a, uint32_t ad_b, uint64_t len_b) {
  const uint64_t m = 65521u, s1a = ad_a & 0xffffu, s2a = ad_a >> 16, s1b = ad_b & 0xffffu, s2b = ad_b >> 16;
  const uint64_t s2 = (s2a + s2b + (len_b % m) * ((s1a + m - 1) % m)) % m;
  const uint64_t s1 = (s1a + s1b + m - 1) % m;
  return (uint32_t)((s2 << 16) | s1);
}

// ---- the container's header ----
struct Head {
  int32_t status = ZH_OK;
  bool need = false;  // the end of the input cuts it short
  uint32_t fmt = 0;
  uint64_t body = 0;  // its length
};
// The checks of zh_unwrap_kernel (zh_inflate.hip) in its order.  whole: the input is the whole stream, and the length
// rules are that kernel's; otherwise every check waits until the bytes it reads are there.
Head read_head(const uint8_t* s, uint64_t len, int fmt, bool whole) {
  Head h;
  if (fmt == ZH_DF_DETECT) {  // zippy.nim:108-125
    if (!whole && len < 4) {
      h.need = true;
      return h;
    }
    if ((!whole || len > 18) && len >= 4 && s[0] == 31 && s[1] == 139 && s[2] == 8 && (s[3] & 0xe0) == 0)
      fmt = ZH_DF_GZIP;
    else if ((!whole || len > 6) && len >= 2 && (s[0] & 0x0f) == 8 && (s[0] >> 4) <= 7 && (((uint32_t)s[0] * 256u) + s[1]) % 31u == 0)
      fmt = ZH_DF_ZLIB;
    else {
      h.status = ZH_ERR_DETECT;
      return h;
    }
  }
  h.fmt = (uint32_t)fmt;
  if (fmt == ZH_DF_GZIP) {  // gzip.nim:9-66
    if (whole ? len < 18 : len < 10) {
      h.status = whole ? (int32_t)ZH_ERR_INVALID_BUFFER : (int32_t)ZH_OK;
      h.need = !whole;
      return h;
    }
    const uint8_t flg = s[3];
    if (s[0] != 31 || s[1] != 139) h.status = ZH_ERR_GZIP_ID;
    else if (s[2] != 8) h.status = ZH_ERR_UNSUPPORTED_METHOD;
    else if (flg & 0xe0) h.status = ZH_ERR_RESERVED_FLAGS;
    else if (flg & 4) h.status = ZH_ERR_UNSUPPORTED_FLAGS;  // FEXTRA
    if (h.status != ZH_OK) return h;
    uint64_t p = 10;
    for (int field = 0; field < 2; field++) {  // FNAME, FCOMMENT
      if (flg & (field == 0 ? 8 : 16)) {
        while (p < len && s[p] != 0) p++;
        if (p >= len) {
          h.status = whole ? (int32_t)ZH_ERR_INVALID_BUFFER : (int32_t)ZH_OK;
          h.need = !whole;
          return h;
        }
        p++;
      }
    }
    if (flg & 2) {  // FHCRC: skipped, not verified (gzip.nim:55-59)
      if (whole ? p + 2 >= len : p + 2 > len) {
        h.status = whole ? (int32_t)ZH_ERR_INVALID_BUFFER : (int32_t)ZH_OK;
        h.need = !whole;
        return h;
      }
      p += 2;
    }
    if (whole && p + 8 >= len) h.status = ZH_ERR_INVALID_BUFFER;
    h.body = p;
  } else if (fmt == ZH_DF_ZLIB) {  // zippy.nim:130-150
    if (whole ? len < 6 : len < 2) {
      h.status = whole ? (int32_t)ZH_ERR_INVALID_BUFFER : (int32_t)ZH_OK;
      h.need = !whole;
      return h;
    }
    const uint8_t cmf = s[0], flg = s[1];
    if ((cmf & 0x0f) != 8) h.status = ZH_ERR_UNSUPPORTED_METHOD;
    else if ((cmf >> 4) > 7) h.status = ZH_ERR_COMPRESSION_INFO;
    else if ((((uint32_t)cmf * 256u) + flg) % 31u != 0) h.status = ZH_ERR_INVALID_HEADER;
    else if (flg & 0x20) h.status = ZH_ERR_PRESET_DICT;
    h.body = 2;
  } else if (fmt != ZH_DF_DEFLATE) {
    h.status = ZH_ERR_INVALID_FORMAT;
  }
  return h;
}

inline uint32_t le32(const uint8_t* t) { return t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24); }
inline uint32_t be32(const uint8_t* t) { return ((uint32_t)t[0] << 24) | (t[1] << 16) | (t[2] << 8) | t[3]; }
inline uint32_t trailer_bytes(uint32_t fmt) { return fmt == ZH_DF_GZIP ? 8u : fmt == ZH_DF_ZLIB ? 4u : 0u; }
// gzip.nim:80-88, zippy.nim:152-162 (zh_verify_kernel)
int32_t check_trailer(const uint8_t* t, uint32_t fmt, uint32_t check, uint64_t total_out) {
  if (fmt == ZH_DF_GZIP) {
    if (le32(t) != check) return ZH_ERR_CHECKSUM;
    if (le32(t + 4) != (uint32_t)(total_out & 0xffffffffu)) return ZH_ERR_SIZE;
  } else if (fmt == ZH_DF_ZLIB) {
    if (be32(t) != check) return ZH_ERR_CHECKSUM;
  }
  return ZH_OK;
}

// a state: the header and, behind it, the window
void* make_state(const zh_resume_header& h, const uint8_t* win_a, size_t len_a, const uint8_t* win_b, size_t len_b) {
  uint8_t* blob = (uint8_t*)malloc(sizeof(h) + len_a + len_b);
  if (!blob) return nullptr;
  memcpy(blob, &h, sizeof(h));
  if (len_a) memcpy(blob + sizeof(h), win_a, len_a);
  if (len_b) memcpy(blob + sizeof(h) + len_a, win_b, len_b);
  return blob;
}
// what can be said of a state without decoding (include/zippy_hip.h)
bool state_sound(const void* state, size_t len, zh_resume_header& h) {
  if (len < sizeof(h)) return false;
  memcpy(&h, state, sizeof(h));
  return memcmp(h.magic, ZH_RESUME_MAGIC, 8) == 0 && h.version == ZH_RESUME_VERSION && h.data_format >= ZH_DF_ZLIB &&
         h.data_format <= ZH_DF_DEFLATE && h.phase >= 1 && h.phase <= 2 && h.bit_skip <= 7 &&
         (h.phase == 1 || h.bit_skip == 0) && h.win_len == std::min<uint64_t>(h.total_out, ZH_FRAG_SIZE) &&
         len == sizeof(h) + h.win_len && h.reserved[0] == 0 && h.reserved[1] == 0;
}

struct Live {  // a stream that decodes in this call
  size_t i;
  zh_resume_header h;  // where it stands (a new stream: behind its container's header)
  uint64_t body;       // the first byte of srcs[i] the decoder reads
  uint64_t cap;        // the bytes its slot holds behind the window
  uint64_t slot;       // the window's place in its group's scratch; the output follows it
};

}  // namespace

static_assert(sizeof(zh_resume_header) == 64, "the state's layout is the header's");

// The call; `cleared`: the output arrays have been set (what they hold from then on is the library's to free)
static int resume_run(zh_ctx* ctx, const void* const* srcs, const size_t* lens, size_t n, int data_format,
                      const void* const* states, const size_t* state_lens, const uint64_t* max_out, const uint8_t* last,
                      void** dsts, size_t* dst_lens, size_t* consumed, void** new_states, size_t* new_state_lens,
                      int32_t* why, int32_t* statuses, bool& cleared) {
  if (!ctx || (n && (!srcs || !lens || !max_out || !dsts || !dst_lens || !consumed || !new_states || !new_state_lens ||
                     !why || !statuses)) ||
      (state_lens && !states) || (states && !state_lens))
    return ZH_ERR_ARGUMENT;
  clear_outputs(dsts, dst_lens, statuses, n);
  for (size_t i = 0; i < n; i++) {
    consumed[i] = 0;
    new_states[i] = nullptr;
    new_state_lens[i] = 0;
    why[i] = ZH_RESUME_NEED_INPUT;
  }
  cleared = true;
  if (data_format < ZH_DF_DETECT || data_format > ZH_DF_DEFLATE) {
    for (size_t i = 0; i < n; i++) statuses[i] = ZH_ERR_INVALID_FORMAT;
    return ZH_ERR_INVALID_FORMAT;
  }
  for (size_t i = 0; i < n; i++)
    if ((!srcs[i] && lens[i]) || max_out[i] == 0 || (states && !states[i] && state_lens[i])) return ZH_ERR_ARGUMENT;
  if (!n) return ZH_OK;
  if (n > 0x7fffffffull) return ZH_ERR_ARGUMENT;

  // ---- what the host settles: states, headers, streams that only wait for their trailer ----
  std::vector<Live> live;
  for (size_t i = 0; i < n; i++) {
    const uint8_t* s8 = (const uint8_t*)srcs[i];
    const bool is_last = last && last[i];
    Live v{};
    v.i = i;
    if (states && states[i]) {
      if (!state_sound(states[i], state_lens[i], v.h)) {
        statuses[i] = ZH_ERR_INVALID_BUFFER;
        continue;
      }
      if (v.h.phase == 2) {  // the trailer alone
        const uint32_t tl = trailer_bytes(v.h.data_format);
        if (lens[i] < tl) {
          if (is_last) {
            statuses[i] = ZH_ERR_CHECKSUM;
          } else if (!(new_states[i] = make_state(v.h, (const uint8_t*)states[i] + sizeof(v.h), v.h.win_len, nullptr, 0))) {
            statuses[i] = ZH_ERR_NOMEM;
          } else {
            new_state_lens[i] = state_lens[i];
          }
          continue;
        }
        statuses[i] = check_trailer(s8, v.h.data_format, v.h.check, v.h.total_out);
        if (statuses[i] == ZH_OK) {
          why[i] = ZH_RESUME_DONE;
          consumed[i] = tl;
        }
        continue;
      }
    } else {
      const Head hd = read_head(s8, lens[i], data_format, is_last);
      if (hd.status != ZH_OK) {
        statuses[i] = hd.status;
        continue;
      }
      if (hd.need) continue;  // (NEED_INPUT, nothing consumed, no state)
      memcpy(v.h.magic, ZH_RESUME_MAGIC, 8);
      v.h.version = ZH_RESUME_VERSION;
      v.h.data_format = hd.fmt;
      v.h.phase = 1;
      v.h.check = hd.fmt == ZH_DF_ZLIB ? 1u : 0u;
      v.body = hd.body;
    }
    // deflate cannot expand further: a slot of that size is never full
    const uint64_t avail = lens[i] - v.body;
    v.cap = std::min<uint64_t>(max_out[i], avail > (~0ull >> 12) ? ~0ull : avail * 1032 + 64);
    live.push_back(v);
  }
  const size_t nl = live.size();
  if (!nl) return ZH_OK;

  // ---- the upload: every live stream's bytes and window, each at a multiple of 16 ----
  ZH_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  Trace tr;
  std::vector<const void*> up_src;
  std::vector<uint64_t> up_off, up_len, src_at(nl), win_at(nl);
  uint64_t up_total = 0;
  for (size_t k = 0; k < nl; k++) {
    const Live& v = live[k];
    src_at[k] = up_total;
    up_src.push_back(srcs[v.i]);
    up_off.push_back(up_total);
    up_len.push_back(lens[v.i]);
    up_total = pad16(up_total + lens[v.i]);
    win_at[k] = up_total;
    if (v.h.win_len) {
      up_src.push_back((const uint8_t*)states[v.i] + sizeof(zh_resume_header));
      up_off.push_back(up_total);
      up_len.push_back(v.h.win_len);
      up_total = pad16(up_total + v.h.win_len);
    }
  }
  DevBuf d_src;
  if (dev_alloc(ctx, d_src, up_total + 256) != hipSuccess) return ZH_ERR_NOMEM;
  if (const int st = zhh_upload_slices(ctx, up_src.data(), up_off, up_len, up_total, d_src.p)) return st;
  tr.mark(ctx, "resume: upload");

  // ---- the groups of streams whose slots fit the scratch budget ----
  struct Group {
    uint32_t k0, nk, wclip0, nwclip, piece0, npiece;
  };
  const uint64_t budget = scratch_budget();
  std::vector<ZhBufDesc> bufs(nl);
  std::vector<uint64_t> start_bit(nl);
  std::vector<uint32_t> hist(nl);
  std::vector<uint8_t> lastf(nl);
  std::vector<ZhClipDesc> wclips;
  std::vector<ZhPieceDesc> pieces;
  std::vector<Group> groups;
  Group g{0, 0, 0, 0, 0, 0};
  uint64_t gbytes = 0, gmax = 0;
  for (size_t k = 0; k < nl; k++) {
    Live& v = live[k];
    // (the window ends, and the output starts, at a multiple of 16: the download copies whole vectors)
    const uint64_t front = pad16(v.h.win_len) - v.h.win_len;
    const uint64_t need = pad256(front + v.h.win_len + v.cap + kGatherSlack);
    if (g.nk && gbytes + need > budget) {
      groups.push_back(g);
      gmax = std::max(gmax, gbytes);
      g = Group{(uint32_t)k, 0, (uint32_t)wclips.size(), 0, (uint32_t)pieces.size(), 0};
      gbytes = 0;
    }
    v.slot = gbytes + front;
    ZhBufDesc b = block_decoder_desc(src_at[k], lens[v.i], v.slot, v.h.win_len + v.cap);
    if (pieces.size() + v.cap / ZH_FRAG_SIZE + 1 > 0x7fffffffull) return ZH_ERR_ARGUMENT;
    b.first_piece = (uint32_t)pieces.size();
    for (uint64_t o = 0; o < v.cap; o += ZH_FRAG_SIZE)
      pieces.push_back(ZhPieceDesc{v.slot + v.h.win_len + o, (uint32_t)std::min<uint64_t>(v.cap - o, ZH_FRAG_SIZE), (uint32_t)k, o});
    b.npieces = (uint32_t)pieces.size() - b.first_piece;
    bufs[k] = b;
    start_bit[k] = v.body * 8 + v.h.bit_skip;
    hist[k] = v.h.win_len;
    lastf[k] = last && last[v.i] ? 1 : 0;
    if (v.h.win_len) append_clips(wclips, win_at[k], v.slot, v.h.win_len);
    if (wclips.size() > 0x7fffffffull) return ZH_ERR_ARGUMENT;
    gbytes += need;
    g.nk++;
    g.nwclip = (uint32_t)wclips.size() - g.wclip0;
    g.npiece = (uint32_t)pieces.size() - g.piece0;
  }
  groups.push_back(g);
  gmax = std::max(gmax, gbytes);
  if (groups.size() > 1 && getenv("ZH_TRACE"))
    fprintf(stderr, "zippy_hip: resume scratch for %zu groups of streams (%zu streams)\n", groups.size(), nl);

  ZhBufDesc* d_bufs = nullptr;
  uint64_t *d_start = nullptr, *d_olen = nullptr, *d_bit = nullptr;
  uint32_t *d_hist = nullptr, *piece_crc = nullptr, *piece_adler = nullptr, *piece_len = nullptr, *buf_crc = nullptr,
           *buf_adler = nullptr;
  uint8_t* d_last = nullptr;
  int32_t *d_status = nullptr, *d_why = nullptr;
  ZhClipDesc* d_wclips = nullptr;
  ZhPieceDesc* d_pieces = nullptr;
  Arena ar;
  DevBuf mem, scratch;
  ar.add(d_bufs, nl, bufs.data());
  ar.add(d_start, nl, start_bit.data());
  ar.add(d_hist, nl, hist.data());
  ar.add(d_last, nl, lastf.data());
  ar.add(d_olen, nl);
  ar.add(d_bit, nl);
  ar.add(d_status, nl);
  ar.add(d_why, nl);
  ar.add(buf_crc, nl);
  ar.add(buf_adler, nl);
  ar.add(d_wclips, wclips.size(), wclips.data());
  ar.add(d_pieces, pieces.size(), pieces.data());
  ar.add(piece_crc, pieces.size());
  ar.add(piece_adler, pieces.size());
  ar.add(piece_len, pieces.size());
  ar.pad(256);
  if (ar.alloc(ctx, mem) != hipSuccess || dev_alloc(ctx, scratch, gmax + 256) != hipSuccess) {
    (void)hipGetLastError();
    ctx->last_error = "hipMalloc(resume)";
    return ZH_ERR_NOMEM;
  }
  ZH_HIP(ctx, hipMemsetAsync(ar.base, 0, ar.size, s));
  ZH_HIP(ctx, ar.upload(s));
  ar.bind();

  std::vector<uint64_t> olen(nl), bit(nl);
  std::vector<int32_t> ost(nl), owhy(nl);
  std::vector<uint32_t> crc(nl), adler(nl);
  for (const Group& q : groups) {
    zh_launch_range_clip(s, d_src.p, scratch.p, d_wclips + q.wclip0, q.nwclip);
    ZhInflateArgs ia = block_decoder_args(d_bufs + q.k0, d_start + q.k0, q.nk, d_olen + q.k0, d_status + q.k0);
    ia.single_block = 0;
    zh_launch_resume_inflate(s, d_src.p, scratch.p, ia, ZhResume{d_hist + q.k0, d_last + q.k0, d_bit + q.k0, d_why + q.k0});
    // (a piece's `buf` counts from the call's first live stream: the lengths come in whole)
    zh_launch_checksum_pieces(s, ctx->cktabs, scratch.p, d_pieces + q.piece0, q.npiece, d_olen, 1, 1, piece_crc + q.piece0,
                              piece_adler + q.piece0, piece_len + q.piece0);
    zh_launch_checksum_combine(s, ctx->cktabs, d_bufs + q.k0, q.nk, piece_crc, piece_adler, piece_len, 1, 1,
                               buf_crc + q.k0, buf_adler + q.k0);
    ZH_HIP(ctx, hipGetLastError());
    ZH_HIP(ctx, hipMemcpyAsync(olen.data() + q.k0, d_olen + q.k0, q.nk * 8ull, hipMemcpyDeviceToHost, s));
    ZH_HIP(ctx, hipMemcpyAsync(bit.data() + q.k0, d_bit + q.k0, q.nk * 8ull, hipMemcpyDeviceToHost, s));
    ZH_HIP(ctx, hipMemcpyAsync(ost.data() + q.k0, d_status + q.k0, q.nk * 4ull, hipMemcpyDeviceToHost, s));
    ZH_HIP(ctx, hipMemcpyAsync(owhy.data() + q.k0, d_why + q.k0, q.nk * 4ull, hipMemcpyDeviceToHost, s));
    ZH_HIP(ctx, hipMemcpyAsync(crc.data() + q.k0, buf_crc + q.k0, q.nk * 4ull, hipMemcpyDeviceToHost, s));
    ZH_HIP(ctx, hipMemcpyAsync(adler.data() + q.k0, buf_adler + q.k0, q.nk * 4ull, hipMemcpyDeviceToHost, s));
    ZH_HIP(ctx, hipStreamSynchronize(s));
    tr.mark(ctx, "resume: decode");
    // the group's data, before the next group takes the scratch
    std::vector<uint64_t> doff(q.nk), dlen(q.nk);
    std::vector<char> take(q.nk);
    std::vector<void*> gd(q.nk, nullptr);
    std::vector<size_t> gl(q.nk, 0);
    std::vector<int32_t> gs(q.nk, ZH_OK);
    for (uint32_t j = 0; j < q.nk; j++) {
      const Live& v = live[q.k0 + j];
      doff[j] = v.slot + v.h.win_len;
      dlen[j] = std::min<uint64_t>(olen[q.k0 + j], v.cap);
      take[j] = ost[q.k0 + j] == ZH_OK && dlen[j] != 0;
    }
    if (const int e = zhh_download(ctx, scratch.p, q.nk, doff, dlen, take, gd.data(), gl.data(), gs.data())) {
      for (void* p : gd) free(p);
      return e;
    }
    tr.mark(ctx, "resume: download");

    // ---- the group's streams settled: trailer, running checksum, the state to come back with ----
    for (uint32_t j = 0; j < q.nk; j++) {
      const size_t k = q.k0 + j;
      const Live& v = live[k];
      const size_t i = v.i;
      const uint8_t* s8 = (const uint8_t*)srcs[i];
      uint8_t* data = (uint8_t*)gd[j];
      const uint64_t made = take[j] ? dlen[j] : 0;
      auto fail = [&](int32_t st) {
        free(data);
        statuses[i] = st;
      };
      if (ost[k] != ZH_OK || gs[j] != ZH_OK) {
        fail(ost[k] != ZH_OK ? ost[k] : gs[j]);
        continue;
      }
      zh_resume_header h = v.h;
      h.total_out += made;
      if (h.data_format == ZH_DF_GZIP) h.check = crc32_join(h.check, crc[k], made);
      else if (h.data_format == ZH_DF_ZLIB) h.check = adler32_join(h.check, adler[k], made);
      uint64_t used = bit[k] / 8;
      h.bit_skip = (uint32_t)(bit[k] & 7u);
      int32_t w = owhy[k];
      bool done = false;
      if (w == ZH_RESUME_DONE) {
        const uint32_t tl = trailer_bytes(h.data_format);
        used = (bit[k] + 7) / 8;
        h.bit_skip = 0;
        if (used + tl > lens[i]) {
          if (lastf[k]) {
            fail(ZH_ERR_CHECKSUM);
            continue;
          }
          h.phase = 2;
          w = ZH_RESUME_NEED_INPUT;
        } else {
          const int32_t st = check_trailer(s8 + used, h.data_format, h.check, h.total_out);
          if (st != ZH_OK) {
            fail(st);
            continue;
          }
          used += tl;
          done = true;
        }
      }
      h.total_in += used;
      if (!done) {
        const uint32_t wl = (uint32_t)std::min<uint64_t>(h.total_out, ZH_FRAG_SIZE);
        const uint64_t from_new = std::min<uint64_t>(made, wl), from_old = wl - from_new;
        h.win_len = wl;
        const uint8_t* old_win = v.h.win_len ? (const uint8_t*)states[i] + sizeof(h) : nullptr;
        void* blob = make_state(h, old_win ? old_win + (v.h.win_len - from_old) : nullptr, from_old,
                                data ? data + (made - from_new) : nullptr, from_new);
        if (!blob) {
          fail(ZH_ERR_NOMEM);
          continue;
        }
        new_states[i] = blob;
        new_state_lens[i] = sizeof(h) + wl;
      }
      dsts[i] = data;
      dst_lens[i] = made;
      consumed[i] = used;
      why[i] = w;
    }
  }
  return ZH_OK;
}

// A call that fails as a whole hands nothing out: whatever the groups before the failure had settled is freed.
extern "C" int zh_uncompress_resume_batch(zh_ctx* ctx, const void* const* srcs, const size_t* lens, size_t n,
                                          int data_format, const void* const* states, const size_t* state_lens,
                                          const uint64_t* max_out, const uint8_t* last, void** dsts, size_t* dst_lens,
                                          size_t* consumed, void** new_states, size_t* new_state_lens, int32_t* why,
                                          int32_t* statuses) {
  bool cleared = false;
  const int rc = resume_run(ctx, srcs, lens, n, data_format, states, state_lens, max_out, last, dsts, dst_lens, consumed,
                            new_states, new_state_lens, why, statuses, cleared);
  if (rc != ZH_OK && cleared)
    for (size_t i = 0; i < n; i++) {
      free(dsts[i]);
      free(new_states[i]);
      dsts[i] = new_states[i] = nullptr;
      dst_lens[i] = new_state_lens[i] = consumed[i] = 0;
    }
  return rc;
}
