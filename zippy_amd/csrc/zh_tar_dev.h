// What the two batch tarball readers share (zh_tar_open_batch.hip: extractAll of tarballs.nim; zh_tar_read_batch.hip:
// Tarball.open of tarballs_v1.nim): the images of a call on the device -- the plain ones uploaded at 512-byte aligned
// offsets, every gzip member decoded by ONE sized uncompress plan --, the index space of their 512-byte blocks, the
// string fields of a header held 8 bytes a lane, the reduction of the headers' statuses to one per tarball, and the
// host stages around each file's own kernels: tar_stage (upload, decode), tar_nodes, tar_results (parse, reduce, the
// records on the host), tar_fetch (the decoded images on the host), tar_reader_of.
// The kernel has internal linkage: each file that includes this header launches its own copy.
#pragma once
#include "zh_walk.h"

namespace {

// One tarball of the walk.  All tarballs of a call share one index space of 512-byte blocks ("nodes"): this one's
// are [blk0, blk0 + nblk), nblk = ceil(len / 512), followed by its END node blk0 + nblk, which points to itself.
struct ZhTarImg {
  const uint8_t* data;  // device address of the uncompressed image, 8-byte aligned, readable up to len + 16
  uint64_t len;
  uint32_t blk0, nblk;
};

__device__ __forceinline__ uint32_t find_img(const ZhTarImg* __restrict__ imgs, uint32_t n_img, uint32_t node) {
  uint32_t lo = 0, hi = n_img;  // the last image whose blk0 <= node
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (imgs[mid].blk0 <= node)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// bits [a, a + n) of the header as a mask over this lane's eight bytes [8 * lane, + 8)
__device__ __forceinline__ uint32_t lane_span(uint32_t lane, uint32_t a, uint32_t n) {
  const uint32_t lo = lane * 8, hi = lo + 8;
  const uint32_t s = a > lo ? a - lo : 0u, e = a + n < hi ? (a + n > lo ? a + n - lo : 0u) : 8u;
  return e > s ? ((1u << e) - 1u) & ~((1u << s) - 1u) : 0u;
}
// $(slice).cstring: the length of the NUL-terminated field [a, a + n); zm = this lane's zero-byte mask
__device__ __forceinline__ uint32_t field_len(uint32_t zm, uint32_t lane, uint32_t a, uint32_t n) {
  const uint32_t m = zm & lane_span(lane, a, n);
  const uint64_t hit = __ballot(m != 0);
  const uint32_t src = hit ? (uint32_t)__ffsll((unsigned long long)hit) - 1u : 0u;
  const uint32_t mm = __shfl(m, (int)src);
  return hit ? src * 8 + (uint32_t)__ffs(mm) - 1u - a : n;
}

// One workgroup per tarball: its headers are the ordinals [ord[blk0], ord[END]); the first of them whose status is
// not ZH_OK gives the tarball's status, as the serial loop stops there.
__global__ __launch_bounds__(256) void zh_tar_reduce_kernel(const ZhTarImg* __restrict__ imgs,
                                                            const uint32_t* __restrict__ ord,
                                                            const int32_t* __restrict__ hstat,
                                                            uint32_t* __restrict__ ranges,
                                                            int32_t* __restrict__ tstat) {
  __shared__ uint32_t wave_min[4];
  const ZhTarImg g = imgs[blockIdx.x];
  const uint32_t first = ord[g.blk0], end = ord[g.blk0 + g.nblk];
  uint32_t best = 0xffffffffu;
  for (uint32_t i = first + threadIdx.x; i < end && best == 0xffffffffu; i += 256)
    if (hstat[i] != ZH_OK) best = i;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) best = min(best, (uint32_t)__shfl_xor(best, m));
  if (zh_lane() == 0) wave_min[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    best = min(min(wave_min[0], wave_min[1]), min(wave_min[2], wave_min[3]));
    tstat[blockIdx.x] = best == 0xffffffffu ? ZH_OK : hstat[best];
    ranges[2 * blockIdx.x] = first;
    ranges[2 * blockIdx.x + 1] = end;
  }
}

inline uint32_t gzip_isize(const uint8_t* src, size_t len) {
  const uint8_t* t = src + len - 4;
  return (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
}

// A tarball of the walk: where its bytes are on the device, who owns them on the host
struct TarWalk {
  size_t t;  // its place in the call
  const uint8_t* d_data;
  uint64_t len;
  int host = -1;  // index into TarStage::own of the host copy a .tar.gz's reader will own
  int slot = -1;  // ... or the decode slot it is still to be fetched from
};
// The images of a call on the device.
struct TarStage {
  DevBuf d_in, d_dec, d_redo;
  std::vector<TarWalk> walk;
  HostBufs own;
  std::vector<uint64_t> doff, olen;  // the decode slots: where in d_dec, how many bytes came out
};

// Upload the images `plain` (at 512-byte aligned offsets) and `gz` (behind them; each at least 18 bytes long) in one
// transfer and decode every gzip member through one sized plan, ISIZE as the slot (gzip.nim:72-76 trustSize; CRC-32
// and ISIZE are verified).  s.walk: the plain images, then the members that decoded; statuses[t] of a member that did
// not is the decoder's.
inline int tar_stage(zh_ctx* ctx, const void* const* images, const size_t* lens, const std::vector<size_t>& plain,
                     const std::vector<size_t>& gz, int32_t* statuses, Trace& tr, const char* what_upload,
                     const char* what_decode, TarStage& s) {
  int st;
  std::vector<const void*> up_src;
  std::vector<uint64_t> up_off, up_len;
  uint64_t o = 0;
  for (size_t t : plain) {
    up_src.push_back(images[t]);
    up_off.push_back(o);
    up_len.push_back(lens[t]);
    o += (lens[t] + 511) & ~(uint64_t)511;
  }
  for (size_t t : gz) {
    up_src.push_back(images[t]);
    up_off.push_back(o);
    up_len.push_back(lens[t]);
    o += (lens[t] + 255) & ~(uint64_t)255;
  }
  if (dev_alloc(ctx, s.d_in, o + 512) != hipSuccess) return ZH_ERR_NOMEM;
  if ((st = zhh_upload_slices(ctx, up_src.data(), up_off, up_len, o, s.d_in.p))) return st;
  tr.mark(ctx, what_upload);
  for (size_t k = 0; k < plain.size(); k++) s.walk.push_back({plain[k], s.d_in.p + up_off[k], lens[plain[k]]});

  const size_t n_gz = gz.size();
  std::vector<uint64_t> dcap(n_gz);
  s.doff.assign(n_gz, 0);
  s.olen.assign(n_gz, 0);
  if (!n_gz) return ZH_OK;
  std::vector<uint64_t> soff(up_off.begin() + plain.size(), up_off.end()),
      slen(up_len.begin() + plain.size(), up_len.end());
  uint64_t total = 0;
  for (size_t k = 0; k < n_gz; k++) {
    const size_t t = gz[k];
    dcap[k] = std::min<uint64_t>(gzip_isize((const uint8_t*)images[t], lens[t]), (uint64_t)lens[t] * 1032 + 64);
    s.doff[k] = total;
    total += (dcap[k] + 511) & ~(uint64_t)511;
  }
  if (dev_alloc(ctx, s.d_dec, total + 512) != hipSuccess) return ZH_ERR_NOMEM;
  PlanGuard pg;
  std::vector<int32_t> ost(n_gz);
  if ((st = zh_plan_uncompress(ctx, n_gz, soff.data(), slen.data(), s.doff.data(), dcap.data(), ZH_DF_GZIP, &pg.p)) ||
      (st = zh_plan_run(pg.p, s.d_in.p, s.d_dec.p)) || (st = zh_plan_results(pg.p, s.olen.data(), ost.data())))
    return st;
  tr.mark(ctx, what_decode);
  // A member that outgrew its ISIZE (4 GiB and more, or damaged) takes zh_tar_open's own route, the host call that
  // retries at the expansion bound: its status is that call's, its image comes back to the device for the walk.
  std::vector<size_t> redo;
  for (size_t k = 0; k < n_gz; k++) {
    if (ost[k] == ZH_ERR_DST_TOO_SMALL)
      redo.push_back(k);
    else if (ost[k] != ZH_OK)
      statuses[gz[k]] = ost[k];
    else
      s.walk.push_back({gz[k], s.d_dec.p + s.doff[k], s.olen[k], -1, (int)k});
  }
  if (redo.empty()) return ZH_OK;
  const size_t nr = redo.size();
  std::vector<const void*> rsrc(nr);
  std::vector<size_t> rlen(nr), rout(nr);
  std::vector<uint64_t> rhint(nr);
  std::vector<void*> rdst(nr, nullptr);
  std::vector<int32_t> rst(nr);
  for (size_t j = 0; j < nr; j++) {
    rsrc[j] = images[gz[redo[j]]];
    rlen[j] = lens[gz[redo[j]]];
    rhint[j] = gzip_isize((const uint8_t*)rsrc[j], rlen[j]);
  }
  st = zh_uncompress_batch_sized(ctx, rsrc.data(), rlen.data(), nr, ZH_DF_GZIP, rhint.data(), rdst.data(), rout.data(),
                                 rst.data(), nullptr);
  s.own.p = rdst;
  if (st) return st;
  std::vector<const void*> hsrc;
  std::vector<size_t> hlen, hwalk;
  for (size_t j = 0; j < nr; j++) {
    if (rst[j] != ZH_OK) {
      statuses[gz[redo[j]]] = rst[j];
      continue;
    }
    hwalk.push_back(s.walk.size());
    s.walk.push_back({gz[redo[j]], nullptr, rout[j], (int)j, -1});
    hsrc.push_back(rdst[j]);
    hlen.push_back(rout[j]);
  }
  if (!hsrc.empty()) {
    std::vector<uint64_t> hoff, hlen64;
    if ((st = zhh_upload(ctx, hsrc.data(), hlen.data(), hsrc.size(), s.d_redo, hoff, hlen64))) return st;
    for (size_t j = 0; j < hwalk.size(); j++) s.walk[hwalk[j]].d_data = s.d_redo.p + hoff[j];
  }
  return ZH_OK;
}

// The walk's index space: imgs[k] of s.walk[k], all nodes of the call, and the rounds of pointer doubling -- after
// `rounds` rounds every node up to 2^rounds - 1 steps from a start is marked; a chain has at most max_blk.
inline int tar_nodes(const std::vector<TarWalk>& walk, std::vector<ZhTarImg>& imgs, uint32_t* n_nodes,
                     uint32_t* rounds) {
  uint64_t n = 0, max_blk = 0;
  imgs.resize(walk.size());
  for (size_t k = 0; k < walk.size(); k++) {
    const uint64_t nblk = (walk[k].len + 511) >> 9;
    if (n + nblk + 1 >= 0xffffffffull) return ZH_ERR_ARGUMENT;  // (2 TiB of images in one call)
    imgs[k] = ZhTarImg{walk[k].d_data, walk[k].len, (uint32_t)n, (uint32_t)nblk};
    n += nblk + 1;
    max_blk = std::max(max_blk, nblk);
  }
  uint32_t r = 0;
  while ((1ull << r) < max_blk + 1) r++;
  *n_nodes = (uint32_t)n;
  *rounds = r;
  return ZH_OK;
}

// What the device found, on the host (in a buffer of s.own): the records of all headers in walk order, their 256-byte
// pool slots, and per tarball of s.walk its range of headers and its status
template <class Rec>
struct TarResults {
  const Rec* recs;
  const uint8_t* pool;
  const uint32_t* ranges;
  const int32_t* tstat;
};
// launch_parse(recs, pool, hstat) launches the caller's parse kernel over the n_hdr headers the walk listed; the
// reduction follows, and everything but the headers' statuses comes back in one download.
template <class Rec, class Parse>
inline int tar_results(zh_ctx* ctx, TarStage& s, const Walk& w, const ZhTarImg* dimgs, size_t n_walk, uint32_t n_hdr,
                       Parse launch_parse, TarResults<Rec>& r) {
  Rec* d_recs;
  uint32_t *d_pool, *d_ranges;
  int32_t *d_tstat, *d_hstat;
  Arena out;
  out.add(d_recs, n_hdr);
  out.add(d_pool, (size_t)n_hdr * 64);
  out.add(d_ranges, n_walk * 2);
  out.add(d_tstat, n_walk);
  const size_t out_bytes = out.size;  // (what comes back: the arrays so far)
  out.add(d_hstat, n_hdr);
  DevBuf d_out;
  if (out.alloc(ctx, d_out, 256) != hipSuccess) return ZH_ERR_NOMEM;
  out.bind();
  const uint32_t* const ord = w.ord;
  if (n_hdr) launch_parse(d_recs, d_pool, d_hstat);
  hipLaunchKernelGGL(zh_tar_reduce_kernel, dim3((uint32_t)n_walk), dim3(256), 0, ctx->stream, dimgs, ord,
                     (const int32_t*)d_hstat, d_ranges, d_tstat);
  ZH_HIP(ctx, hipGetLastError());
  void* h_out = nullptr;
  size_t got = 0;
  int32_t dst_st = ZH_OK;
  if (const int st = zhh_download(ctx, d_out.p, 1, {0}, {out_bytes}, {1}, &h_out, &got, &dst_st)) {
    free(h_out);
    return st;
  }
  s.own.p.push_back(h_out);
  if (dst_st) return dst_st;
  r = TarResults<Rec>{out.host(h_out, d_recs), reinterpret_cast<const uint8_t*>(out.host(h_out, d_pool)),
                      out.host(h_out, d_ranges), out.host(h_out, d_tstat)};
  return ZH_OK;
}

// The decoded images of the tarballs that opened (tstat[k] of s.walk[k]) come to the host: walk[k].host says where.
inline int tar_fetch(zh_ctx* ctx, TarStage& s, const int32_t* tstat) {
  const size_t n_gz = s.doff.size(), n_walk = s.walk.size();
  std::vector<char> take(n_gz, 0);
  for (size_t k = 0; k < n_walk; k++)
    if (s.walk[k].slot >= 0 && tstat[k] == ZH_OK) take[(size_t)s.walk[k].slot] = 1;
  std::vector<void*> idst(n_gz, nullptr);
  std::vector<size_t> ilen(n_gz, 0);
  std::vector<int32_t> ist(n_gz, ZH_OK);
  const int st =
      n_gz ? zhh_download(ctx, s.d_dec.p, n_gz, s.doff, s.olen, take, idst.data(), ilen.data(), ist.data()) : ZH_OK;
  const size_t base = s.own.p.size();
  s.own.p.insert(s.own.p.end(), idst.begin(), idst.end());
  if (st) return st;
  for (size_t k = 0; k < n_walk; k++)
    if (s.walk[k].slot >= 0 && tstat[k] == ZH_OK) {
      if (ist[(size_t)s.walk[k].slot]) return ist[(size_t)s.walk[k].slot];  // (allocation)
      s.walk[k].host = (int)(base + (size_t)s.walk[k].slot);
    }
  return ZH_OK;
}

// The empty reader of s.walk[k], *data its image: the caller's (borrowed), or the host copy it owns from here on
inline zh_tar_reader* tar_reader_of(TarStage& s, size_t k, const void* const* images, const uint8_t** data) {
  const TarWalk& w = s.walk[k];
  const bool borrowed = w.host < 0;
  void* const owned = borrowed ? nullptr : s.own.p[(size_t)w.host];
  *data = (const uint8_t*)(borrowed ? images[w.t] : owned);
  zh_tar_reader* r = zh_tar_reader_new(owned, *data, (size_t)w.len);
  if (r && !borrowed) s.own.p[(size_t)w.host] = nullptr;
  return r;
}
struct CloseAll {  // the readers made so far: closed when the call fails
  std::vector<zh_tar_reader*>& v;
  bool armed = true;
  ~CloseAll() {
    if (armed)
      for (zh_tar_reader* r : v) zh_tar_close(r);
  }
};

}  // namespace
