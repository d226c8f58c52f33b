// The host arithmetic that the two range reads share (zh_ranges.hip: zh_uncompress_ranges, zh_plan_uncompress_ranges
// over a block index of bit_off / out_off; zh_bgzf.hip: zh_bgzf_read_ranges over a member index of coff / uoff):
//   range_geometry   pread's arithmetic and the binary search: the entries that hold a range's first and last byte
//   RangeSpans       the compressed bytes the live ranges need, merged owner by owner, each merged span at a multiple
//                    of 16 of one upload
//   append_clips     an edge block's bytes on their way from the scratch into a slot, in pieces of kClipChunk
//   hand_out         the tail of a host call: one download, or nothing handed out at all
// What an entry is, which index is sound and where a span's bytes begin and end are the caller's: they come in as the
// entry type, a callable and plain numbers.  Host code only.
#pragma once
#include "zh_host.h"

namespace {

// What a range comes to before anything is decoded: its status if that is settled already, its clipped length, and
// the entries k0 .. k1 of its stream's own list (blocks, members) that hold its first and last byte (none: k0 > k1).
struct RangeGeo {
  int32_t fixed = ZH_OK;
  uint64_t off = 0, end = 0;  // clipped
  size_t k0 = 1, k1 = 0;
};

// pread's arithmetic and the binary search; ZH_ERR_ARGUMENT for a caller's bug.  Stream s's entries are
// index[first[s] .. first[s + 1]), the last of them the closing entry; uoff(entry): its place in the uncompressed
// data; sound(s, entries, count): what can be said of the list without decoding, asked once a stream, when a range
// first asks -- the ranges of a stream whose list is not sound are ZH_ERR_INVALID_BUFFER.
template <class Entry, class Sound, class Uoff>
int range_geometry(size_t n_streams, const Entry* index, const size_t* first, size_t n_ranges, const uint64_t* rs,
                   const uint64_t* ro, const uint64_t* rl, Sound sound, Uoff uoff, std::vector<RangeGeo>& geo) {
  if (n_ranges && (!rs || !ro || !rl)) return ZH_ERR_ARGUMENT;
  if (n_streams && !first) return ZH_ERR_ARGUMENT;
  for (size_t s = 0; s < n_streams; s++)
    if (first[s + 1] < first[s]) return ZH_ERR_ARGUMENT;
  if (n_streams && first[n_streams] > first[0] && !index) return ZH_ERR_ARGUMENT;
  for (size_t r = 0; r < n_ranges; r++)
    if (rs[r] >= n_streams) return ZH_ERR_ARGUMENT;
  std::vector<signed char> ok(n_streams, -1);  // (checked when a range first asks)
  geo.assign(n_ranges, RangeGeo{});
  for (size_t r = 0; r < n_ranges; r++) {
    const size_t s = (size_t)rs[r];
    const Entry* e = index + first[s];
    const size_t ne = first[s + 1] - first[s];
    if (ok[s] < 0) ok[s] = sound(s, e, ne) ? 1 : 0;
    RangeGeo& g = geo[r];
    if (!ok[s]) {
      g.fixed = ZH_ERR_INVALID_BUFFER;
      continue;
    }
    const uint64_t total = uoff(e[ne - 1]);
    if (ro[r] >= total || !rl[r]) continue;
    g.off = ro[r];
    g.end = rl[r] > total - ro[r] ? total : ro[r] + rl[r];  // (off + len may not fit 64 bits)
    auto holds = [&](uint64_t byte) {  // the entry k with uoff[k] <= byte < uoff[k + 1]
      return (size_t)(std::upper_bound(e, e + ne, byte, [&](uint64_t v, const Entry& x) { return v < uoff(x); }) - e) - 1;
    };
    g.k0 = holds(g.off);
    g.k1 = holds(g.end - 1);
  }
  return ZH_OK;
}

// Only the compressed bytes the ranges need go over the link: add() takes the bytes [lo, hi) of owner s (a stream, an
// image) once a live range; place() sorts them, makes one span of those of an owner that overlap or touch, and gives
// every merged span the next multiple of 16 in one device buffer -- at most 15 bytes of padding a span.  sp / soff /
// slen are zhh_upload_slices' arguments, up_total the bytes the link carries; the spare bytes behind them are the
// caller's choice.
struct RangeSpans {
  struct Span {
    uint64_t owner, lo, hi, dev;
  };
  std::vector<Span> spans;
  std::vector<const void*> sp;
  std::vector<uint64_t> soff, slen;
  uint64_t up_total = 0;
  void add(uint64_t owner, uint64_t lo, uint64_t hi) { spans.push_back(Span{owner, lo, hi, 0}); }
  void place(const void* const* srcs) {
    std::sort(spans.begin(), spans.end(),
              [](const Span& a, const Span& b) { return a.owner != b.owner ? a.owner < b.owner : a.lo < b.lo; });
    size_t m = 0;
    for (size_t i = 0; i < spans.size(); i++) {
      if (m && spans[m - 1].owner == spans[i].owner && spans[i].lo <= spans[m - 1].hi)
        spans[m - 1].hi = std::max(spans[m - 1].hi, spans[i].hi);
      else
        spans[m++] = spans[i];
    }
    spans.resize(m);
    sp.resize(m);
    soff.resize(m);
    slen.resize(m);
    for (size_t i = 0; i < m; i++) {
      up_total = (up_total + 15) & ~(uint64_t)15;
      spans[i].dev = soff[i] = up_total;
      slen[i] = spans[i].hi - spans[i].lo;
      sp[i] = (const uint8_t*)srcs[spans[i].owner] + spans[i].lo;
      up_total += slen[i];
    }
  }
  // what was added for a range lies in one merged span: the last one of its owner that starts at or before `lo`
  const Span& holding(uint64_t owner, uint64_t lo) const {
    const auto it = std::upper_bound(spans.begin(), spans.end(), lo, [owner](uint64_t v, const Span& x) {
      return x.owner != owner ? owner < x.owner : v < x.lo;
    });
    return *(it - 1);
  }
};

// The bytes scratch[src, src + len) of an edge block on their way to d_dst[dst, dst + len): pieces of at most
// kClipChunk bytes -- one workgroup never moves a whole block -- that end where the slot's offset is a multiple of 16:
// with d_dst aligned, bytes go singly at a clip's two ends only.
inline void append_clips(std::vector<ZhClipDesc>& clips, uint64_t src, uint64_t dst, uint64_t len) {
  for (uint64_t a = 0; a < len;) {
    const uint64_t d = dst + a;
    uint64_t n = std::min<uint64_t>(len - a, kClipChunk);
    if (n == kClipChunk && ((d + n) & 15u)) n -= (d + n) & 15u;
    clips.push_back(ZhClipDesc{src + a, d, (uint32_t)n, 0});
    a += n;
  }
}

// The tail of a host call: the slots [doff[k], + olen[k]) of d_dst whose st[k] is ZH_OK come down into fresh buffers,
// and every status is handed out.  When that fails -- the device, or no memory -- nothing is: the buffers made so far
// are freed and the three arrays read as they did before anything was handed out.
inline int hand_out(zh_ctx* ctx, const uint8_t* d_dst, const std::vector<uint64_t>& doff,
                    const std::vector<uint64_t>& olen, std::vector<int32_t> st, void** dsts, size_t* dst_lens,
                    int32_t* statuses) {
  const size_t n = st.size();
  std::vector<char> take(n);
  for (size_t k = 0; k < n; k++) take[k] = st[k] == ZH_OK;
  if (const int e = zhh_download(ctx, d_dst, n, doff, olen, take, dsts, dst_lens, st.data())) {
    for (size_t k = 0; k < n; k++) free(dsts[k]);
    clear_outputs(dsts, dst_lens, statuses, n);
    return e;
  }
  for (size_t k = 0; k < n; k++) statuses[k] = st[k];
  return ZH_OK;
}

}  // namespace
