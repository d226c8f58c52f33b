// Byte-range reads from block-indexed streams (zh_plan_uncompress_ranges, zh_uncompress_ranges): what a block index
// is for.  A range of the uncompressed data touches a run of deflate blocks; the blocks that lie wholly inside it are
// decoded straight into the range's slot, the one or two that its ends cut into go through plan-owned scratch and
// are clipped into place.  The decoder is zh_inflate_kernel (zh_inflate.hip), one wave pair a block, as in
// zh_plan_uncompress_indexed; this file holds the clip and reduce kernels, the plan over the ranges, and the host call
// that sends only the compressed bytes the ranges need over the link.  The arithmetic it has in common with
// zh_bgzf_read_ranges -- the geometry, the merged spans of the upload, the cut of a clip into pieces, the tail that
// hands the results out -- is zh_range_host.h's; what a block index adds (bit offsets, stream_index_ok) stays here.
#include "zh_gather.h"
#include "zh_range_host.h"

// One workgroup per piece of a clip: scratch[src, src + len) -> d_dst[dst, dst + len).  Stores of 16 bytes to aligned
// addresses, the source gathered at whatever alignment it has (src & 15 is one value for the whole piece); byte
// stores for the up to 15 bytes in front of the first aligned address and behind the last.  Runs whether or not the
// block decoded: zh_ranges_reduce_kernel decides what the slot is worth.  The kernel keeps its own workgroup-wide loop
// in 32-bit offsets from the slot's pointer (d_dst is the caller's, at any alignment): through zh_gather.h's
// copy_range with a stride of 256 threads it took 5 % longer.
__global__ __launch_bounds__(256) void zh_range_clip_kernel(const uint8_t* __restrict__ d_scratch,
                                                            uint8_t* __restrict__ d_dst,
                                                            const ZhClipDesc* __restrict__ clips) {
  const ZhClipDesc c = clips[blockIdx.x];
  uint8_t* d = d_dst + c.dst;
  uint32_t head = (16u - (uint32_t)((uintptr_t)d & 15u)) & 15u;
  if (head > c.len) head = c.len;
  const uint32_t nv = (c.len - head) >> 4, tail0 = head + (nv << 4);
  if (threadIdx.x < head) d[threadIdx.x] = d_scratch[c.src + threadIdx.x];
  if (tail0 + threadIdx.x < c.len) d[tail0 + threadIdx.x] = d_scratch[c.src + tail0 + threadIdx.x];
  const uint64_t s = c.src + head;
  for (uint32_t j = threadIdx.x; j < nv; j += 256u)
    *reinterpret_cast<Chunk16*>(d + head + 16u * j) = gather16(d_scratch, s + 16ull * j);
}

// One wave per range: the lowest block (in index order) that failed, or did not make exactly the bytes its index
// entries promise, decides; ZH_OK and ZH_ERR_DST_TOO_SMALL of such a block read ZH_ERR_INVALID_BUFFER, as in
// zh_segments_reduce_kernel.  A range of no blocks is what the plan said of it.
__global__ __launch_bounds__(64) void zh_ranges_reduce_kernel(ZhRangesArgs a) {
  const uint32_t r = blockIdx.x;
  const unsigned lane = zh_lane();
  const int32_t fixed = a.fixed_status[r];
  if (fixed != ZH_OK) {
    if (lane == 0) {
      a.status[r] = fixed;
      a.out_len[r] = fixed == ZH_ERR_DST_TOO_SMALL ? a.clip_len[r] : 0;
    }
    return;
  }
  const uint32_t b0 = a.first_block[r], b1 = a.first_block[r + 1];
  uint32_t bad = 0xffffffffu;
  for (uint32_t j = b0 + lane; j < b1; j += 64u) {
    const uint32_t k = a.order[j];
    if ((a.blk_status[k] != ZH_OK || a.blk_len[k] != a.bufs[k].dst_cap) && j < bad) bad = j;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bad = min(bad, (uint32_t)__shfl_xor(bad, o, 64));
  if (lane != 0) return;
  if (bad == 0xffffffffu) {
    a.status[r] = ZH_OK;
    a.out_len[r] = a.clip_len[r];
  } else {
    const int32_t st = a.blk_status[a.order[bad]];
    a.status[r] = (st == ZH_OK || st == ZH_ERR_DST_TOO_SMALL) ? (int32_t)ZH_ERR_INVALID_BUFFER : st;
    a.out_len[r] = 0;
  }
}

extern "C" void zh_launch_range_clip(hipStream_t stream, const uint8_t* d_scratch, uint8_t* d_dst,
                                     const ZhClipDesc* clips, uint32_t nclips) {
  if (!nclips) return;
  hipLaunchKernelGGL(zh_range_clip_kernel, dim3(nclips), dim3(256), 0, stream, d_scratch, d_dst, clips);
}
extern "C" void zh_launch_ranges_reduce(hipStream_t stream, ZhRangesArgs a) {
  if (!a.nranges) return;
  hipLaunchKernelGGL(zh_ranges_reduce_kernel, dim3(a.nranges), dim3(64), 0, stream, a);
}

// ---------------------------------------------------------------------------
// geometry
// ---------------------------------------------------------------------------
namespace {

// Where a range's compressed bytes are: the block that starts at bit b of its stream is decoded from bit b - 8 * skip
// of d_src[off .. off + len).
struct RangeSrc {
  uint64_t off, len, skip;
};

// the bytes that hold the bits in front of `bit` (no sum that could pass 2^64: a closing entry may say anything)
inline uint64_t bytes_up_to(uint64_t bit) { return bit / 8 + ((bit & 7) != 0); }

// A stream's index passes the static checks, and no block promises more than deflate can expand its bytes to
// (1032 bytes a byte, the guard of zh_uncompress_indexed, a block at a time: the scratch is sized by the promises).
bool stream_index_ok(const zh_block_entry* e, size_t n, uint64_t src_len) {
  if (n > 0xfffffffeull || !block_index_sound(e, n, src_len)) return false;
  for (size_t k = 0; k + 1 < n; k++) {
    const uint64_t bytes = bytes_up_to(e[k + 1].bit_off) - e[k].bit_off / 8;
    if (bytes > (~0ull - 64) / 1032) continue;
    if (e[k + 1].out_off - e[k].out_off > bytes * 1032 + 64) return false;
  }
  return true;
}

// range_geometry (zh_range_host.h) over a block index: the entry's place is out_off, the verdict stream_index_ok's
int ranges_geometry(size_t n_streams, const uint64_t* src_len, const zh_block_entry* index, const size_t* first,
                    size_t n_ranges, const uint64_t* rs, const uint64_t* ro, const uint64_t* rl,
                    std::vector<RangeGeo>& geo) {
  if (n_streams && !src_len) return ZH_ERR_ARGUMENT;
  return range_geometry(
      n_streams, index, first, n_ranges, rs, ro, rl,
      [&](size_t s, const zh_block_entry* e, size_t ne) { return stream_index_ok(e, ne, src_len[s]); },
      [](const zh_block_entry& x) { return x.out_off; }, geo);
}

// The plan over ranges whose geometry and compressed bytes are known.  dst_cap: null where every slot is as long as
// its clipped range (the host call).
int ranges_build(zh_ctx* ctx, const zh_block_entry* index, const size_t* first, size_t n_ranges, const uint64_t* rs,
                 std::vector<RangeGeo>& geo, const std::vector<RangeSrc>& src, const uint64_t* dst_off,
                 const uint64_t* dst_cap, zh_plan** out) {
  if (n_ranges > 0x7fffffffull) return ZH_ERR_ARGUMENT;
  ZH_HIP(ctx, hipSetDevice(ctx->device));
  const uint64_t budget = scratch_budget();
  std::vector<ZhBufDesc> ip, sc;        // blocks decoded in place / into scratch
  std::vector<uint64_t> ip_bit, sc_bit;
  std::vector<uint32_t> order, first_block(n_ranges + 1);  // (a scratch block's position: 0x80000000 | its number, until all are counted)
  std::vector<ZhClipDesc> clips;
  std::vector<ZhRangesPlan::Group> groups;
  std::vector<int32_t> fixed(n_ranges);
  std::vector<uint64_t> clip_len(n_ranges);
  ZhRangesPlan::Group g{0, 0, 0, 0, 0, 0};
  uint64_t gbytes = 0, gmax = 0;
  bool gany = false;
  for (size_t r = 0; r < n_ranges; r++) {
    RangeGeo& q = geo[r];
    clip_len[r] = q.end - q.off;
    if (q.fixed == ZH_OK && dst_cap && dst_cap[r] < clip_len[r]) q.fixed = ZH_ERR_DST_TOO_SMALL;
    fixed[r] = q.fixed;
    first_block[r] = (uint32_t)order.size();
    if (q.fixed != ZH_OK || q.k0 > q.k1) continue;
    const zh_block_entry* e = index + first[rs[r]];
    // the range's edge blocks first: what they take of the scratch decides whether the range opens a new group
    auto edge_bytes = [&](size_t k) -> uint64_t {  // (k0 and k1 hold a byte of the range each: neither is empty)
      const uint64_t bs = e[k].out_off, be = e[k + 1].out_off;
      return bs < q.off || be > q.end ? (be - bs + kGatherSlack + 255) & ~(uint64_t)255 : 0;
    };
    const uint64_t need = edge_bytes(q.k0) + (q.k1 > q.k0 ? edge_bytes(q.k1) : 0);
    if (gany && gbytes + need > budget) {
      groups.push_back(g);
      gmax = std::max(gmax, gbytes);
      g = ZhRangesPlan::Group{(uint32_t)ip.size(), 0, (uint32_t)sc.size(), 0, (uint32_t)clips.size(), 0};
      gbytes = 0;
    }
    gany = true;
    if (order.size() + (q.k1 - q.k0 + 1) > 0x7fffffffull) return ZH_ERR_ARGUMENT;
    for (size_t k = q.k0; k <= q.k1; k++) {
      const uint64_t bs = e[k].out_off, be = e[k + 1].out_off;
      if (be == bs) continue;  // (an empty block: nothing of it lies in any range)
      const uint64_t bit = e[k].bit_off - 8 * src[r].skip;
      if (bs >= q.off && be <= q.end) {
        order.push_back((uint32_t)ip.size());
        ip.push_back(block_decoder_desc(src[r].off, src[r].len, dst_off[r] + (bs - q.off), be - bs));
        ip_bit.push_back(bit);
        continue;
      }
      order.push_back(0x80000000u | (uint32_t)sc.size());
      sc.push_back(block_decoder_desc(src[r].off, src[r].len, gbytes, be - bs));
      sc_bit.push_back(bit);
      const uint64_t lo = std::max(q.off, bs), hi = std::min(q.end, be);
      append_clips(clips, gbytes + (lo - bs), dst_off[r] + (lo - q.off), hi - lo);
      gbytes += (be - bs + kGatherSlack + 255) & ~(uint64_t)255;
    }
    if (clips.size() > 0x7fffffffull) return ZH_ERR_ARGUMENT;
    g.nip = (uint32_t)ip.size() - g.ip0;
    g.nsc = (uint32_t)sc.size() - g.sc0;
    g.nclip = (uint32_t)clips.size() - g.clip0;
  }
  first_block[n_ranges] = (uint32_t)order.size();
  if (gany) {
    groups.push_back(g);
    gmax = std::max(gmax, gbytes);
  }
  const size_t nip = ip.size(), nsc = sc.size(), nb = nip + nsc, nc = clips.size();
  for (uint32_t& o : order)
    if (o & 0x80000000u) o = (uint32_t)nip + (o & 0x7fffffffu);
  ip.insert(ip.end(), sc.begin(), sc.end());
  ip_bit.insert(ip_bit.end(), sc_bit.begin(), sc_bit.end());
  if (groups.size() > 1 && getenv("ZH_TRACE"))
    fprintf(stderr, "zippy_hip: scratch for %zu groups of ranges (%zu ranges)\n", groups.size(), n_ranges);

  zh_plan* p = new zh_plan;
  p->ctx = ctx;
  p->is_compress = false;
  p->n = n_ranges;
  p->rg.reset(new ZhRangesPlan);
  ZhRangesPlan& R = *p->rg;
  R.n_in_place = (uint32_t)nip;
  R.n_scratch = (uint32_t)nsc;
  R.groups = std::move(groups);
  ZhRangesArgs& a = R.a;
  Arena ar;
  ar.add(a.bufs, nb, ip.data());
  ar.add(a.start_bit, nb, ip_bit.data());
  ar.add(a.blk_len, nb);
  ar.add(a.blk_status, nb);
  ar.add(a.first_block, n_ranges + 1, first_block.data());
  ar.add(a.order, nb, order.data());
  ar.add(a.fixed_status, n_ranges, fixed.data());
  ar.add(a.clip_len, n_ranges, clip_len.data());
  ar.add(a.clips, nc, clips.data());
  ar.add(p->out_len, n_ranges);
  ar.add(p->status, n_ranges);
  ar.pad(256);
  if (ar.alloc(ctx, R.arena) != hipSuccess || (gmax && dev_alloc(ctx, R.scratch, gmax + 256) != hipSuccess)) {
    (void)hipGetLastError();
    ctx->last_error = "hipMalloc(ranges plan)";
    zh_plan_destroy(p);
    return ZH_ERR_NOMEM;
  }
  hipStream_t s = ctx->stream;
  hipError_t up = hipMemsetAsync(ar.base, 0, ar.size, s);
  if (up == hipSuccess) up = ar.upload(s);
  if (up == hipSuccess) up = hipStreamSynchronize(s);
  if (up != hipSuccess) {
    ctx->last_error = std::string("plan upload: ") + hipGetErrorString(up);
    zh_plan_destroy(p);
    return ZH_ERR_DEVICE;
  }
  ar.bind();
  a.out_len = p->out_len;
  a.status = p->status;
  a.nranges = (uint32_t)n_ranges;
  *out = p;
  return ZH_OK;
}

}  // namespace

extern "C" int zh_plan_uncompress_ranges(zh_ctx* ctx, size_t n_streams, const uint64_t* src_off, const uint64_t* src_len,
                                         const zh_block_entry* index, const size_t* first, size_t n_ranges,
                                         const uint64_t* range_stream, const uint64_t* range_off,
                                         const uint64_t* range_len, const uint64_t* dst_off, const uint64_t* dst_cap,
                                         zh_plan** out) {
  if (!ctx || !out) return ZH_ERR_ARGUMENT;
  *out = nullptr;
  if ((n_streams && !src_off) || (n_ranges && (!dst_off || !dst_cap))) return ZH_ERR_ARGUMENT;
  std::vector<RangeGeo> geo;
  if (const int st = ranges_geometry(n_streams, src_len, index, first, n_ranges, range_stream, range_off, range_len, geo))
    return st;
  std::vector<RangeSrc> src(n_ranges);
  for (size_t r = 0; r < n_ranges; r++) src[r] = RangeSrc{src_off[range_stream[r]], src_len[range_stream[r]], 0};
  return ranges_build(ctx, index, first, n_ranges, range_stream, geo, src, dst_off, dst_cap, out);
}

// Only the compressed bytes the ranges' blocks occupy go over the link: per range the span [bit_off[k0] / 8,
// ceil(bit_off[k1 + 1] / 8)) of its stream; spans of one stream that overlap or touch are sent once.  Every span
// lands at the next multiple of 16 in one device buffer -- at most 15 bytes of padding a span --, and the link carries
// that buffer from its first byte to the last span's end.
extern "C" int zh_uncompress_ranges(zh_ctx* ctx, const void* const* srcs, const size_t* lens, size_t n_streams,
                                    const zh_block_entry* index, const size_t* first, size_t n_ranges,
                                    const uint64_t* range_stream, const uint64_t* range_off, const uint64_t* range_len,
                                    void** dsts, size_t* dst_lens, int32_t* statuses) {
  if (!ctx || (n_streams && (!srcs || !lens)) || (n_ranges && (!dsts || !dst_lens || !statuses))) return ZH_ERR_ARGUMENT;
  clear_outputs(dsts, dst_lens, statuses, n_ranges);
  for (size_t s = 0; s < n_streams; s++)
    if (!srcs[s] && lens[s]) return ZH_ERR_ARGUMENT;
  std::vector<uint64_t> len64(lens, lens + n_streams);
  std::vector<RangeGeo> geo;
  if (const int st = ranges_geometry(n_streams, len64.data(), index, first, n_ranges, range_stream, range_off,
                                     range_len, geo))
    return st;
  if (!n_ranges) return ZH_OK;
  Trace tr;
  // the spans, merged stream by stream
  RangeSpans up;
  for (size_t r = 0; r < n_ranges; r++) {
    const RangeGeo& q = geo[r];
    if (q.fixed != ZH_OK || q.k0 > q.k1) continue;
    const size_t s = (size_t)range_stream[r];
    const zh_block_entry* e = index + first[s];
    up.add(s, e[q.k0].bit_off / 8, std::min<uint64_t>(bytes_up_to(e[q.k1 + 1].bit_off), lens[s]));
  }
  up.place(srcs);
  const uint64_t up_total = up.up_total;
  ZH_HIP(ctx, hipSetDevice(ctx->device));
  DevBuf d_src;
  if (dev_alloc(ctx, d_src, up_total + 256) != hipSuccess) return ZH_ERR_NOMEM;
  if (const int st = zhh_upload_slices(ctx, up.sp.data(), up.soff, up.slen, up_total, d_src.p)) return st;
  tr.mark(ctx, "ranges: upload");
  // every range's span lies in one merged span: the last one of its stream that starts at or before it
  std::vector<RangeSrc> src(n_ranges, RangeSrc{0, 0, 0});
  std::vector<uint64_t> doff(n_ranges), dcap(n_ranges);
  uint64_t dst_total = 0;
  for (size_t r = 0; r < n_ranges; r++) {
    const RangeGeo& q = geo[r];
    doff[r] = dst_total;
    dcap[r] = q.end - q.off;
    dst_total += (dcap[r] + 255) & ~(uint64_t)255;
    if (q.fixed != ZH_OK || q.k0 > q.k1) continue;
    const uint64_t s = range_stream[r];
    const RangeSpans::Span& x = up.holding(s, index[first[s] + q.k0].bit_off / 8);
    src[r] = RangeSrc{x.dev, x.hi - x.lo, x.lo};
  }
  DevBuf d_dst;
  if (dev_alloc(ctx, d_dst, dst_total + 256) != hipSuccess) return ZH_ERR_NOMEM;
  PlanGuard pg;
  int st = ranges_build(ctx, index, first, n_ranges, range_stream, geo, src, doff.data(), nullptr, &pg.p);
  if (st) return st;
  if ((st = zh_plan_run(pg.p, d_src.p, d_dst.p))) return st;
  std::vector<uint64_t> olen(n_ranges);
  std::vector<int32_t> ost(n_ranges);
  if ((st = zh_plan_results(pg.p, olen.data(), ost.data()))) return st;
  ctx->rg_uploaded = up_total;
  tr.mark(ctx, "ranges: decode");
  if ((st = hand_out(ctx, d_dst.p, doff, olen, ost, dsts, dst_lens, statuses))) return st;
  tr.mark(ctx, "ranges: download");
  return ZH_OK;
}

extern "C" int zh_debug_range_stats(zh_ctx* ctx, uint64_t* uploaded_bytes, uint64_t* blocks_in_place,
                                    uint64_t* blocks_via_scratch) {
  if (!ctx) return ZH_ERR_ARGUMENT;
  if (uploaded_bytes) *uploaded_bytes = ctx->rg_uploaded;
  if (blocks_in_place) *blocks_in_place = ctx->rg_in_place;
  if (blocks_via_scratch) *blocks_via_scratch = ctx->rg_via_scratch;
  return ZH_OK;
}
