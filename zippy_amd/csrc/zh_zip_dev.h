// What the two batch zip readers share (zh_zip_open_batch.hip: openZipArchive of ziparchives.nim; zh_zip_read_batch.hip:
// ZipArchive.open of ziparchives_v1.nim): little-endian field loads, the bounds rule, the per-archive first-failure
// reduction, the guard of a call's readers, and everything behind the tables -- the file entries of a call ("slots")
// are decoded, copied and verified by zip_extract (one uncompress plan, the checksum kernels, zh_zip_finish_kernel),
// come to the host by zip_download, and the few that outgrew their slots are decoded again by zip_redo.  The kernels
// have internal linkage: each file that includes this header launches its own copy.
#pragma once
#include "zh_gather.h"
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

struct Readers {  // the readers of the call until it succeeds
  std::vector<zh_zip_reader*> r;
  ~Readers() {
    for (zh_zip_reader* q : r) zh_zip_close(q);
  }
};

uint64_t round_up8(uint64_t x) { return (x + 7) & ~(uint64_t)7; }

constexpr uint64_t kSlice = 32768;  // bytes of a stored entry a wave copies at most

// One file entry that is extracted and verified: `img` among the call's images, `rec` the caller's record of it.
// The caller lays the slots out: [dst, + cap) of the output, 8-byte aligned, an image's slots next to each other.
struct ZipSlot {
  size_t img;
  uint32_t rec;
  uint64_t src, src_len;  // its data in the upload buffer
  uint64_t dst, cap;
  uint32_t want_crc, want_len;
  int32_t local_status;  // not ZH_OK: nothing to extract, this is the entry's status
  uint32_t method;       // the local header's: 8 deflated, else stored
};
// ... for zh_zip_finish_kernel
struct ZhZipFin {
  uint64_t src, dst, len;  // a stored entry: len bytes from upload buffer + src to output buffer + dst
  uint32_t want_crc, want_len;
  int32_t local_status;
  uint32_t deflated;  // 1: result `idx` of the plan; 0: stored entry `idx` of the checksum launch
  uint32_t idx;
};
struct ZhZipFinTask {
  uint64_t lo, hi;  // bytes [lo, hi) of the entry's data
  uint32_t entry, first;
};

// One wave per task (four a workgroup): a slice of a stored entry's bytes goes from its image to its (differently
// aligned) slot by zh_gather.h's copy_range.  The wave of an entry's
// first task also settles the entry, by the first of these that applies: a local header that failed; the decoder's
// status (deflated entries: the plan's status, length and CRC-32); the CRC-32 against the header's; with check_len,
// the length against the header's.  elen (if given): the entry's length, 0 when it failed.
__global__ __launch_bounds__(256) void zh_zip_finish_kernel(const uint8_t* __restrict__ d_in, uint8_t* __restrict__ d_out,
                                                            const ZhZipFin* __restrict__ fins,
                                                            const ZhZipFinTask* __restrict__ tasks, uint32_t n_tasks,
                                                            const int32_t* __restrict__ plan_st,
                                                            const uint64_t* __restrict__ plan_len,
                                                            const uint32_t* __restrict__ plan_crc,
                                                            const uint32_t* __restrict__ stored_crc, uint32_t check_len,
                                                            int32_t* __restrict__ est, uint64_t* __restrict__ elen) {
  const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = zh_lane();
  if (w >= n_tasks) return;
  const ZhZipFinTask t = tasks[w];
  const ZhZipFin e = fins[t.entry];
  if (t.first && lane == 0) {
    int32_t st = e.local_status;
    uint64_t len = 0;
    if (st == ZH_OK) {
      st = e.deflated ? plan_st[e.idx] : ZH_OK;
      const uint32_t crc = e.deflated ? plan_crc[e.idx] : stored_crc[e.idx];
      len = e.deflated ? plan_len[e.idx] : e.len;
      if (st == ZH_OK && crc != e.want_crc) st = ZH_ERR_ZIP_CRC;
      if (st == ZH_OK && check_len && len != e.want_len) st = ZH_ERR_ZIP_SIZE;
      if (st != ZH_OK) len = 0;
    }
    est[t.entry] = st;
    if (elen) elen[t.entry] = len;
  }
  copy_range(d_out, e.dst + t.lo, e.dst + t.hi, d_in, e.src - e.dst, lane);  // (source byte = slot byte + delta)
}

// One decode, the stored entries and every verdict: the slots' data goes from the upload buffer d_in into their places
// in d_out (out_total bytes, allocated here).  eranges[2k .. 2k + 1]: image k's slots.  On ZH_OK est[j] is slot j's
// status, elen[j] (if wanted) its length, ebad[k] the first slot of image k that failed (kNone: none).  The trace
// marks are "<what>: decode" and "<what>: finish".
inline int zip_extract(zh_ctx* ctx, Trace& tr, const char* what, const std::vector<ZipSlot>& slots,
                       const std::vector<uint32_t>& eranges, const uint8_t* in, uint64_t out_total, bool check_len,
                       DevBuf& d_out, std::vector<int32_t>& est, std::vector<uint64_t>* elen,
                       std::vector<uint32_t>& ebad) {
  const size_t n_slot = slots.size(), n_img = eranges.size() / 2;
  int st;
  hipStream_t s = ctx->stream;
  const dim3 wg(256);
  std::vector<ZhZipFin> fins(n_slot);
  std::vector<ZhZipFinTask> tasks;
  std::vector<uint64_t> p_soff, p_slen, p_doff, p_dcap;
  std::vector<ZhPieceDesc> pieces;
  std::vector<ZhBufDesc> sbufs;
  for (size_t j = 0; j < n_slot; j++) {
    const ZipSlot& sl = slots[j];
    ZhZipFin& f = fins[j];
    f = ZhZipFin{sl.src, sl.dst, 0, sl.want_crc, sl.want_len, sl.local_status, 0, 0};
    uint64_t copy = 0;
    if (sl.local_status == ZH_OK && sl.method == 8) {
      f.deflated = 1;
      f.idx = (uint32_t)p_soff.size();
      p_soff.push_back(sl.src);
      p_slen.push_back(sl.src_len);
      p_doff.push_back(sl.dst);
      p_dcap.push_back(sl.cap);
    } else if (sl.local_status == ZH_OK) {
      f.len = copy = sl.src_len;
      f.idx = (uint32_t)sbufs.size();
      ZhBufDesc b;
      memset(&b, 0, sizeof(b));
      b.src_off = sl.src;
      b.src_len = copy;
      b.first_piece = (uint32_t)pieces.size();
      for (uint64_t o = 0; o < copy; o += ZH_FRAG_SIZE)
        pieces.push_back(ZhPieceDesc{sl.src + o, (uint32_t)std::min<uint64_t>(copy - o, ZH_FRAG_SIZE), f.idx, o});
      b.npieces = (uint32_t)pieces.size() - b.first_piece;
      sbufs.push_back(b);
    }
    uint32_t first = 1;
    for (uint64_t o = 0; first || o < copy; o += kSlice, first = 0)
      tasks.push_back(ZhZipFinTask{o, std::min<uint64_t>(copy, o + kSlice), (uint32_t)j, first});
  }
  const size_t n_def = p_soff.size(), n_sto = sbufs.size(), n_piece = pieces.size(), n_task = tasks.size();
  if (n_task >= 0xffffffffull || n_piece >= 0xffffffffull) return ZH_ERR_ARGUMENT;
  DevBuf d_fin;
  if (dev_alloc(ctx, d_out, out_total + 256) != hipSuccess) return ZH_ERR_NOMEM;
  const ZhZipFin* d_fins;
  const ZhZipFinTask* d_tasks;
  const ZhBufDesc* d_sbufs;
  const ZhPieceDesc* d_pieces;
  const uint32_t* d_er;
  uint32_t *d_pcrc, *d_pad, *d_plen, *d_scrc, *d_sad, *d_ebad, *d_eany;
  int32_t* d_est;
  uint64_t* d_elen;
  Arena fa;
  fa.add(d_fins, n_slot, fins.data());
  fa.add(d_tasks, n_task, tasks.data());
  fa.add(d_sbufs, n_sto, sbufs.data());
  fa.add(d_pieces, n_piece, pieces.data());
  fa.add(d_er, n_img * 2, eranges.data());
  const size_t fa_in = fa.size;  // (what is uploaded: the arrays so far)
  fa.add(d_pcrc, n_piece);
  fa.add(d_pad, n_piece);
  fa.add(d_plen, n_piece);
  fa.add(d_scrc, n_sto);
  fa.add(d_sad, n_sto);
  fa.add(d_est, n_slot);
  fa.add(d_elen, elen ? n_slot : 0);
  fa.add(d_ebad, n_img);
  fa.add(d_eany, n_img);
  if (fa.alloc(ctx, d_fin, 256) != hipSuccess) return ZH_ERR_NOMEM;
  fa.bind();
  if (!elen) d_elen = nullptr;
  // (plain pointers from here on: a launch must not take the guard of a buffer or of the plan along)
  uint8_t* const outp = d_out.p;
  {
    std::vector<uint8_t> h(fa_in);
    fa.gather(h.data());
    const void* src = h.data();
    if ((st = zhh_upload_slices(ctx, &src, {0}, {(uint64_t)fa_in}, fa_in, fa.base))) return st;
  }
  const std::string mark = std::string(what) + ": ";
  PlanGuard pg;
  if (n_def) {
    if ((st = zh_plan_uncompress(ctx, n_def, p_soff.data(), p_slen.data(), p_doff.data(), p_dcap.data(),
                                 ZH_DF_DEFLATE, &pg.p)) ||
        (st = zh_plan_request_crc32(pg.p, 1)))
      return st;
    if (tr.on) zh_plan_set_profiling(pg.p, 1);
    if ((st = zh_plan_run(pg.p, in, outp))) return st;
    if (tr.on) {
      const char* names[64];
      float ms[64];
      const int nk = zh_plan_kernel_times(pg.p, names, ms, 64);
      for (int i = 0; i < nk && i < 64; i++) fprintf(stderr, "[zh]   plan kernel %-24s %8.3f ms\n", names[i], ms[i]);
    }
  }
  tr.mark(ctx, (mark + "decode").c_str());
  zh_launch_checksum_pieces(s, ctx->cktabs, in, d_pieces, (uint32_t)n_piece, nullptr, 1, 0, d_pcrc, d_pad, d_plen);
  zh_launch_checksum_combine(s, ctx->cktabs, d_sbufs, (uint32_t)n_sto, d_pcrc, d_pad, d_plen, 1, 0, d_scrc, d_sad);
  const int32_t* const plan_st = n_def ? zh_plan_device_statuses(pg.p) : nullptr;
  const uint64_t* const plan_len = n_def ? zh_plan_device_lens(pg.p) : nullptr;
  const uint32_t* const plan_crc = n_def ? pg.p->buf_crc : nullptr;
  hipLaunchKernelGGL(zh_zip_finish_kernel, dim3(((uint32_t)n_task + 3) / 4), wg, 0, s, in, outp, d_fins, d_tasks,
                     (uint32_t)n_task, plan_st, plan_len, plan_crc, (const uint32_t*)d_scrc, check_len ? 1u : 0u, d_est,
                     d_elen);
  hipLaunchKernelGGL(zh_zip_reduce_kernel, dim3((uint32_t)n_img), wg, 0, s, d_er, (const int32_t*)d_est,
                     (const uint8_t*)nullptr, d_ebad, d_eany);
  ZH_HIP(ctx, hipGetLastError());
  est.assign(n_slot, ZH_OK);
  ebad.assign(n_img, kNone);
  ZH_HIP(ctx, hipMemcpyAsync(est.data(), d_est, n_slot * 4, hipMemcpyDeviceToHost, s));
  if (elen) {
    elen->assign(n_slot, 0);
    ZH_HIP(ctx, hipMemcpyAsync(elen->data(), d_elen, n_slot * 8, hipMemcpyDeviceToHost, s));
  }
  ZH_HIP(ctx, hipMemcpyAsync(ebad.data(), d_ebad, n_img * 4, hipMemcpyDeviceToHost, s));
  ZH_HIP(ctx, hipStreamSynchronize(s));
  tr.mark(ctx, (mark + "finish").c_str());
  return ZH_OK;
}

// One download: image k's block [aoff[k], + alen[k]) of the output, where take[k] is set, into a fresh host buffer.
// blocks[k] is own.p[*blocks_at + k] until a reader takes it.
inline int zip_download(zh_ctx* ctx, const uint8_t* d_out, const std::vector<uint64_t>& aoff,
                        const std::vector<uint64_t>& alen, const std::vector<char>& take, HostBufs& own,
                        std::vector<void*>& blocks, size_t* blocks_at) {
  const size_t n = take.size();
  std::vector<size_t> blen(n, 0);
  std::vector<int32_t> bst(n, ZH_OK);
  const int st = zhh_download(ctx, d_out, n, aoff, alen, take, blocks.data(), blen.data(), bst.data());
  *blocks_at = own.p.size();
  own.p.insert(own.p.end(), blocks.begin(), blocks.end());
  if (st) return st;
  for (size_t k = 0; k < n; k++)
    if (take[k] && bst[k]) return bst[k];  // (allocation)
  return ZH_OK;
}

// The slots whose est is ZH_ERR_DST_TOO_SMALL -- a stream that decodes to more than its header claims -- take
// zh_zip_extract_batch's own route: decoded in full from the host image (himg[k], at up_off[k] of the upload), all of
// the call in one batch (rare: the CRC of these is compared on the host).  Their slot's capacity is the hint: that
// call clamps a hint as the slot was clamped.  est[j] = verdict(j, status, crc, length, buffer) for each; a verdict
// that keeps the buffer sets it to NULL, the others are freed with `own`.  ebad of their images is made anew.
template <class Verdict>
inline int zip_redo(zh_ctx* ctx, Trace& tr, const char* what, const std::vector<ZipSlot>& slots,
                    const std::vector<uint32_t>& eranges, const void* const* himg, const std::vector<uint64_t>& up_off,
                    HostBufs& own, std::vector<int32_t>& est, std::vector<uint32_t>& ebad, Verdict verdict) {
  std::vector<size_t> redo;
  for (size_t j = 0; j < slots.size(); j++)
    if (est[j] == ZH_ERR_DST_TOO_SMALL) redo.push_back(j);
  if (redo.empty()) return ZH_OK;
  const size_t nr = redo.size();
  std::vector<const void*> rsrc(nr);
  std::vector<size_t> rlen(nr), rout(nr);
  std::vector<uint64_t> rhint(nr);
  std::vector<void*> rdst(nr, nullptr);
  std::vector<int32_t> rst(nr);
  std::vector<uint32_t> rcrc(nr);
  for (size_t q = 0; q < nr; q++) {
    const ZipSlot& sl = slots[redo[q]];
    rsrc[q] = (const uint8_t*)himg[sl.img] + (sl.src - up_off[sl.img]);
    rlen[q] = (size_t)sl.src_len;
    rhint[q] = sl.cap;
  }
  const int st = zh_uncompress_batch_sized(ctx, rsrc.data(), rlen.data(), nr, ZH_DF_DEFLATE, rhint.data(), rdst.data(),
                                           rout.data(), rst.data(), rcrc.data());
  const size_t base = own.p.size();
  own.p.insert(own.p.end(), rdst.begin(), rdst.end());
  if (st) return st;
  for (size_t q = 0; q < nr; q++) est[redo[q]] = verdict(redo[q], rst[q], rcrc[q], rout[q], own.p[base + q]);
  for (size_t q = 0; q < nr; q++) {  // the first failing slot of these images, once more
    const size_t k = slots[redo[q]].img;
    if (q && slots[redo[q - 1]].img == k) continue;
    ebad[k] = kNone;
    for (size_t j = eranges[2 * k]; j < eranges[2 * k + 1] && ebad[k] == kNone; j++)
      if (est[j] != ZH_OK) ebad[k] = (uint32_t)j;
  }
  tr.mark(ctx, (std::string(what) + ": redo").c_str());
  return ZH_OK;
}

}  // namespace
