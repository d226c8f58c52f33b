// Reading zip archives the v1 way: ZipArchive.open (src/zippy/ziparchives_v1.nim:105-349 openStreamImpl) for many
// images a call.  The walk starts at byte 0 of an image and goes from record to record over the image's own bytes, so
// the candidates of the walk are found first:
//   zh_sig_scan_kernel    every 16-byte chunk of the upload is read once a pass (count, then write): the positions
//                         whose four bytes are one of the three signatures and lie inside ONE image are the hits,
//                         sorted by position
//   zh_zipr_ranges_kernel per image: its range of hits; an image whose byte 0 is no hit is settled here
//   zh_zipr_next_kernel   next[h] for every hit as if a record started there, its target found among the image's hits
//                         by binary search; a record that fails, an end record and a target that is no hit end a chain
//   zh_walk_double_kernel the hits reachable from an image's byte 0 ARE its records (zh_walk.h)
//   zh_walk_scan_*        every record's ordinal in walk order, the list of records
//   zh_zipr_parse_kernel  one wave per record: the checks of the loop body in their order; one fixed-size record
//   zh_zip_reduce_kernel  per image: the first record that failed
//   (host)                the tables from the records in walk order (toUnixPath, replacement, the central records'
//                         lookup); the layout of the output; ONE uncompress plan over every deflated local record of
//                         the call, its sources in place in the uploaded images; the first failure in walk order
//   zh_zip_finish_kernel  stored entries copied image -> slot; every record's CRC-32, then its length, held against
//                         its header (zh_zip_dev.h, with the host stages around it)
// The host parses no header byte, compares no CRC and copies no entry.
//
// Scratch: 8 bytes per hit (the list), 20 per node of the walk (a hit, or an image's END node), 4 per 16 KiB of the
// upload (the scan's group sums).  Nothing is kept per image byte.
//
// Every image sits at an 8-byte aligned offset of ONE allocation that ends with 512 spare bytes (the plan reads whole
// aligned words around a source, the stored copy and the scan aligned 16-byte chunks).  The bytes between two images
// and behind the last are stale: a signature there, or one that begins in an image's tail and ends in the padding or
// the next image, is no hit.
//
// That layout and upload, the two passes of the scan with their ZH_TRACE lines, the rounds of doubling and the walk's
// scratch are host code of zh_scan.h (scan_upload, scan_hits, scan_walk_alloc), shared with zh_bgzf.hip;
// zh_walk_rec_ranges_kernel is zh_walk.h's.  This file holds what is zip's: the three kernels on read_head, the tables.
#include <unordered_map>

#include "zh_scan.h"
#include "zh_zip_dev.h"

namespace {

constexpr uint32_t kLocalSig = 0x04034b50u, kCentralSig = 0x02014b50u, kEndSig = 0x06054b50u;
enum : uint8_t { kKindLocal = 1, kKindCentral = 2, kKindEnd = 3 };

// What stands at a position if a record starts there: the checks of openStreamImpl's loop body up to the decoder
// (:115-200, :228-269, :296-319) in their order.  status: the first that failed; next: the position behind the record.
struct ZhZrHead {
  uint64_t next, name_off, data_off;
  uint32_t name_len, csize, usize, crc, external;
  int32_t status;
  uint16_t dos_time, dos_date;
  uint8_t kind, method;
};

// One reached record, for the host
struct ZhZrRec {
  uint64_t pos, name_off, data_off;  // in the image
  uint32_t name_len, csize, usize, crc, external;
  int32_t status, succ_status;  // its own checks; what the walk finds where the next record should start
  uint16_t dos_time, dos_date;
  uint8_t kind, method, backslash, pad;
};

// the scan's predicate (zh_scan.h)
struct ZipSignature {
  static __device__ __forceinline__ bool match(uint32_t v) {
    return (v & 0xffffu) == 0x4b50u && (v == kLocalSig || v == kCentralSig || v == kEndSig);
  }
};

// a record's header at image position pos (p = the image, len its length); see ZhZrHead
__device__ __forceinline__ ZhZrHead read_head(const uint8_t* __restrict__ p, uint64_t len, uint64_t pos) {
  ZhZrHead h{};
  const uint8_t* __restrict__ q = p + pos;
  const uint32_t sig = ld32(q);  // (a hit: its four bytes are inside the image)
  if (sig == kLocalSig) {
    h.kind = kKindLocal;
    if (pos + 30 > len) {
      h.status = ZH_ERR_ARCHIVE_EOF;
      return h;
    }
    const uint32_t flags = ld16(q + 6), method = ld16(q + 8);
    h.dos_time = (uint16_t)ld16(q + 10);
    h.dos_date = (uint16_t)ld16(q + 12);
    h.crc = ld32(q + 14);
    h.csize = ld32(q + 18);
    h.usize = ld32(q + 22);
    h.name_len = ld16(q + 26);
    h.method = (uint8_t)method;
    h.name_off = pos + 30;
    h.data_off = h.name_off + h.name_len + ld16(q + 28);
    h.next = h.data_off + h.csize;
    if (flags & 4u)
      h.status = ZH_ERR_ZIP_DATA_DESCRIPTOR;
    else if (flags & 8u)
      h.status = ZH_ERR_ZIP_DEFLATE64;
    else if (method != 0 && method != 8)
      h.status = ZH_ERR_ZIP_METHOD;
    else if (h.data_off > len || h.next > len)
      h.status = ZH_ERR_ARCHIVE_EOF;
  } else if (sig == kCentralSig) {
    h.kind = kKindCentral;
    if (pos + 46 > len) {
      h.status = ZH_ERR_ARCHIVE_EOF;
      return h;
    }
    h.name_len = ld16(q + 28);
    h.external = ld32(q + 38);
    h.name_off = pos + 46;
    h.next = h.name_off + h.name_len + ld16(q + 30) + ld16(q + 32);
    if (h.next > len) h.status = ZH_ERR_ARCHIVE_EOF;
  } else {
    h.kind = kKindEnd;
    if (pos + 22 > len) {
      h.status = ZH_ERR_ARCHIVE_EOF;
      return h;
    }
    h.next = pos + 22 + ld16(q + 20);
    if (h.next > len) h.status = ZH_ERR_ARCHIVE_EOF;
  }
  return h;
}

}  // namespace

// Per image: ranges[2t .. 2t + 1] = its hits; start[t] = ZH_OK when its byte 0 is a hit, else what the loop's first
// trip says (:115-116, :328-329)
__global__ __launch_bounds__(256) void zh_zipr_ranges_kernel(const ZhZrImg* __restrict__ imgs, uint32_t n_img,
                                                             const uint64_t* __restrict__ hits, uint32_t n_hits,
                                                             uint32_t* __restrict__ ranges, int32_t* __restrict__ start) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_img) return;
  const ZhZrImg g = imgs[t];
  const uint32_t lo = lower_bound(hits, 0, n_hits, g.up_off), hi = lower_bound(hits, lo, n_hits, g.up_off + g.len);
  ranges[2 * t] = lo;
  ranges[2 * t + 1] = hi;
  start[t] = lo < hi && hits[lo] == g.up_off ? ZH_OK : g.len < 4 ? ZH_ERR_ARCHIVE_EOF : ZH_ERR_ZIP_OPEN;
}

// next[b] for every node b: nodes [0, n_hits) are the hits, node n_hits + t is image t's END (its own successor).  A
// hit's successor is the hit at the position behind its record; it is END when the record fails a check of its own,
// when it is an end record, and when that position is no hit -- succ[b] then says what the loop finds there:
// failEOF within the last three bytes (:115-116), failOpen elsewhere (:328-329).  mark[b] = 1 for byte 0 of an image.
__global__ __launch_bounds__(256) void zh_zipr_next_kernel(const uint8_t* __restrict__ d_in,
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
    const ZhZrHead h = read_head(d_in + g.up_off, g.len, pos);
    int32_t sc = ZH_OK;
    nx = n_hits + t;
    if (h.status == ZH_OK && h.kind != kKindEnd) {
      if (h.next + 4 > g.len) {
        sc = ZH_ERR_ARCHIVE_EOF;
      } else {
        const uint32_t hi = ranges[2 * t + 1], k = lower_bound(hits, b + 1, hi, g.up_off + h.next);
        if (k < hi && hits[k] == g.up_off + h.next)
          nx = k;
        else
          sc = ZH_ERR_ZIP_OPEN;
      }
    }
    succ[b] = sc;
    mk = pos == 0 ? 1u : 0u;
  }
  jump[b] = nx;
  mark[b] = mk;
}

// One wave per reached record, in walk order (h = its ordinal in the call, list[h] its node).  The fields are read by
// every lane (the same addresses: one broadcast load each); a local record's name goes over the lanes, which look
// for a backslash (the host converts only the names that have one).
__global__ __launch_bounds__(256) void zh_zipr_parse_kernel(const uint8_t* __restrict__ d_in,
                                                            const ZhZrImg* __restrict__ imgs, uint32_t n_img,
                                                            const uint64_t* __restrict__ hits,
                                                            const uint32_t* __restrict__ list,
                                                            const int32_t* __restrict__ succ, uint32_t n_rec,
                                                            ZhZrRec* __restrict__ recs, int32_t* __restrict__ rstat) {
  const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = zh_lane();
  if (r >= n_rec) return;
  const uint32_t node = list[r];
  const uint64_t at = hits[node];
  const ZhZrImg g = imgs[find_img(imgs, n_img, at)];
  const uint8_t* __restrict__ p = d_in + g.up_off;
  const ZhZrHead h = read_head(p, g.len, at - g.up_off);
  bool slash = false;
  if (h.status == ZH_OK && h.kind == kKindLocal)
    for (uint32_t j = lane; j < h.name_len; j += 64) slash = slash || p[h.name_off + j] == '\\';
  const bool backslash = __ballot(slash) != 0;
  if (lane == 0) {
    ZhZrRec rec{};
    rec.pos = at - g.up_off;
    rec.name_off = h.name_off;
    rec.data_off = h.data_off;
    rec.name_len = h.name_len;
    rec.csize = h.csize;
    rec.usize = h.usize;
    rec.crc = h.crc;
    rec.external = h.external;
    rec.status = h.status;
    rec.succ_status = succ[node];
    rec.dos_time = h.dos_time;
    rec.dos_date = h.dos_date;
    rec.kind = h.kind;
    rec.method = h.method;
    rec.backslash = backslash ? 1 : 0;
    recs[r] = rec;
    rstat[r] = h.status != ZH_OK ? h.status : rec.succ_status;
  }
}

namespace {

// ZipArchive.contents as it grows (an OrderedTable[string, ArchiveEntry]): keys in first-insertion order
struct Table {
  struct Entry {
    std::string key;
    uint32_t rec;  // its last local record
    bool directory = false, in_directory = false;
    uint32_t unix_mode = 0;
  };
  std::vector<Entry> entries;
  std::unordered_map<std::string, size_t> index;
};

}  // namespace

extern "C" int zh_zip_read_batch(zh_ctx* ctx, const void* const* images, const size_t* lens, size_t n_zip,
                                 zh_zip_reader** readers, int32_t* statuses) {
  if (const int e = reader_checks(ctx, images, lens, n_zip, readers, statuses)) return e;
  if (!n_zip) return ZH_OK;

  // ---- 1. the layout of the upload; 2. one upload; 3. the signature scan (zh_scan.h) ----
  Trace tr;
  int st;
  ScanUpload S;
  ScanHits H;
  if ((st = scan_upload(ctx, tr, "zip read", images, lens, n_zip, 22, S))) return st;  // (no record is shorter than the end record)
  if ((st = scan_hits<ZipSignature>(ctx, tr, "zip read", S, H))) return st;
  hipStream_t s = ctx->stream;
  const dim3 wg(256);
  const uint32_t n_img = S.n_img, n_hits = H.n_hits;
  const uint8_t* const in = S.d_in.p;
  const ZhZrImg* const dimgs = S.imgs();
  const uint64_t* const hits = H.hits();

  // ---- 4. the walk ----
  // behind the walk's scratch: what the loop finds behind every hit (succ), every image's range of hits
  const uint32_t rounds = H.rounds, N = n_hits + n_img;
  int32_t* succ;
  uint32_t* hit_ranges;
  Arena ex;
  ex.add(succ, n_hits);
  ex.add(hit_ranges, (size_t)n_img * 2);
  Walk w;
  if ((st = scan_walk_alloc(ctx, S, H, ex, w))) return st;
  uint32_t *const j0 = w.j0, *const mark = w.mark;
  const uint32_t *const ord = w.ord, *const list = w.list;
  // the per-image outputs live in the block that is downloaded with the records (below); the start statuses are
  // written now, so they get a place of their own here
  DevBuf d_start;
  if (dev_alloc(ctx, d_start, (size_t)n_img * 4 + 256) != hipSuccess) return ZH_ERR_NOMEM;
  int32_t* const start = reinterpret_cast<int32_t*>(d_start.p);
  const dim3 node_grid((N + 255) / 256), img_grid((n_img + 255) / 256);
  hipLaunchKernelGGL(zh_zipr_ranges_kernel, img_grid, wg, 0, s, dimgs, n_img, hits, n_hits, hit_ranges, start);
  hipLaunchKernelGGL(zh_zipr_next_kernel, node_grid, wg, 0, s, in, dimgs, n_img, hits, n_hits,
                     (const uint32_t*)hit_ranges, N, j0, mark, succ);
  walk_double(w, rounds, s);
  walk_scan(w, s);
  uint32_t n_rec = 0;
  if ((st = walk_count(ctx, w, &n_rec))) return st;
  tr.mark(ctx, "zip read: reach + scan");

  // ---- 5. the records ----
  ZhZrRec* d_recs;
  uint32_t *d_ranges, *d_bad, *d_any;
  int32_t *d_start_st, *d_rstat;
  Arena out;
  out.add(d_recs, n_rec);
  out.add(d_ranges, (size_t)n_img * 2);
  out.add(d_bad, n_img);
  out.add(d_start_st, n_img);
  const size_t out_bytes = out.size;  // (what comes back: the arrays so far)
  out.add(d_rstat, n_rec);
  out.add(d_any, n_img);
  DevBuf d_rec;
  if (out.alloc(ctx, d_rec, 256) != hipSuccess) return ZH_ERR_NOMEM;
  out.bind();
  if (n_rec)
    hipLaunchKernelGGL(zh_zipr_parse_kernel, dim3((n_rec + 3) / 4), wg, 0, s, in, dimgs, n_img, hits, list,
                       (const int32_t*)succ, n_rec, d_recs, d_rstat);
  hipLaunchKernelGGL(zh_walk_rec_ranges_kernel, img_grid, wg, 0, s, (const uint32_t*)hit_ranges, n_img, ord, d_ranges);
  hipLaunchKernelGGL(zh_zip_reduce_kernel, dim3(n_img), wg, 0, s, (const uint32_t*)d_ranges, (const int32_t*)d_rstat,
                     (const uint8_t*)nullptr, d_bad, d_any);
  ZH_HIP(ctx, hipGetLastError());
  ZH_HIP(ctx, hipMemcpyAsync(d_start_st, start, (size_t)n_img * 4, hipMemcpyDeviceToDevice, s));
  HostBufs own;
  void* h_rec = nullptr;
  {
    size_t got = 0;
    int32_t dst_st = ZH_OK;
    st = zhh_download(ctx, d_rec.p, 1, {0}, {out_bytes}, {1}, &h_rec, &got, &dst_st);
    own.p.push_back(h_rec);
    if (st || dst_st) return st ? st : dst_st;
  }
  const ZhZrRec* const recs = out.host(h_rec, d_recs);
  const uint32_t* const ranges = out.host(h_rec, d_ranges);
  const uint32_t* const first_bad = out.host(h_rec, d_bad);
  const int32_t* const start_st = out.host(h_rec, d_start_st);
  tr.mark(ctx, "zip read: parse + reduce");

  // ---- 6. the tables, from the records in walk order; the layout of the output ----
  // hst[t]: the first failure of the header checks, the central records' lookups and the walk's steps.  A local
  // record in front of it still has its say (decoder, CRC, size): every one of them gets a slot.
  std::vector<Table> tables(n_zip);
  std::vector<int32_t> hst(n_zip, ZH_OK);
  std::vector<ZipSlot> slots;
  std::vector<uint32_t> eranges(2 * n_zip, 0);  // an image's slots
  std::vector<uint64_t> aoff(n_zip, 0), alen(n_zip, 0);
  std::unordered_map<uint32_t, size_t> slot_of;  // a local record's slot
  uint64_t out_total = 0;
  for (size_t t = 0; t < n_zip; t++) {
    eranges[2 * t] = eranges[2 * t + 1] = (uint32_t)slots.size();
    if (start_st[t] != ZH_OK) {
      hst[t] = start_st[t];
      continue;
    }
    const uint8_t* const image = (const uint8_t*)images[t];
    const uint32_t lo = ranges[2 * t], hi = ranges[2 * t + 1];
    // records behind the first that failed on the device are never reached by the serial loop
    const uint32_t stop = first_bad[t] == kNone ? hi : first_bad[t] + 1;
    Table& tab = tables[t];
    out_total = (out_total + 15) & ~(uint64_t)15;  // (the download moves a block 16 bytes at a time)
    aoff[t] = out_total;
    bool ended = false;
    for (uint32_t i = lo; i < stop && hst[t] == ZH_OK && !ended; i++) {
      const ZhZrRec& e = recs[i];
      if (e.status != ZH_OK) {
        hst[t] = e.status;
        break;
      }
      if (e.kind == kKindLocal) {
        // never above the stream's expansion bound: a tiny image cannot claim gigabytes
        const uint64_t cap = e.method == 8 ? std::min<uint64_t>(e.usize, (uint64_t)e.csize * 1032 + 64) : e.csize;
        slot_of[i] = slots.size();
        slots.push_back(ZipSlot{t, i, S.up_off[t] + e.data_off, e.csize, out_total, cap, e.crc, e.usize, ZH_OK, e.method});
        out_total += round_up8(cap);
        std::string key((const char*)image + e.name_off, e.name_len);
        if (e.backslash) std::replace(key.begin(), key.end(), '\\', '/');  // toUnixPath
        const auto it = tab.index.find(key);
        if (it == tab.index.end()) {
          tab.index.emplace(key, tab.entries.size());
          tab.entries.push_back(Table::Entry{std::move(key), i});
        } else {
          tab.entries[it->second] = Table::Entry{std::move(key), i};  // a fresh ArchiveEntry in the key's place
        }
      } else if (e.kind == kKindCentral) {
        const auto it = tab.index.find(std::string((const char*)image + e.name_off, e.name_len));
        if (it == tab.index.end()) {
          hst[t] = ZH_ERR_ZIP_OPEN;
          break;
        }
        Table::Entry& en = tab.entries[it->second];
        if (e.external & 0x10u) en.directory = true;
        en.unix_mode = e.external >> 16;
        en.in_directory = true;
      } else {
        ended = true;
      }
      if (e.succ_status != ZH_OK) hst[t] = e.succ_status;
    }
    if (hst[t] == ZH_OK && !ended) {
      ctx->last_error = "zh_zip_read_batch: a walk that ends nowhere";
      return ZH_ERR_DEVICE;
    }
    eranges[2 * t + 1] = (uint32_t)slots.size();
    alen[t] = out_total - aoff[t];
  }
  const size_t n_slot = slots.size();
  if (n_slot >= 0xffffffffull) return ZH_ERR_ARGUMENT;
  tr.mark(ctx, "zip read: tables");

  // ---- 7. one decode; 8. the stored entries and every verdict ----
  std::vector<int32_t> est, ast(hst);
  std::vector<void*> blocks(n_zip, nullptr);
  size_t blocks_at = 0;
  if (n_slot) {
    DevBuf d_out;
    std::vector<uint32_t> ebad;
    if ((st = zip_extract(ctx, tr, "zip read", slots, eranges, in, out_total, true, d_out, est, nullptr, ebad)))
      return st;
    // A stream that outgrew its slot decodes to more than its header claims: CRC comes before size (:208-217), so it
    // is decoded again in full (zip_redo).  None of them can end well: at best the length is not the header's.
    if ((st = zip_redo(ctx, tr, "zip read", slots, eranges, images, S.up_off, own, est, ebad,
                       [&](size_t j, int32_t rst, uint32_t rcrc, size_t rout, void*&) {
                         const ZipSlot& sl = slots[j];
                         return rst != ZH_OK ? rst : rcrc != sl.want_crc ? ZH_ERR_ZIP_CRC
                                : rout != sl.want_len ? ZH_ERR_ZIP_SIZE : ZH_OK;
                       })))
      return st;
    // every verified record stands in front of its image's hst in walk order
    for (size_t t = 0; t < n_zip; t++)
      if (ebad[t] != kNone) ast[t] = est[ebad[t]];

    // ---- 9. one download: the block of every archive that opened ----
    std::vector<char> take(n_zip, 0);
    for (size_t t = 0; t < n_zip; t++) take[t] = ast[t] == ZH_OK && alen[t] ? 1 : 0;
    if ((st = zip_download(ctx, d_out.p, aoff, alen, take, own, blocks, &blocks_at))) return st;
    tr.mark(ctx, "zip read: download");
  }

  // ---- the readers: the table's keys in first-insertion order, each with its last local record ----
  Readers made;
  made.r.assign(n_zip, nullptr);
  for (size_t t = 0; t < n_zip; t++) {
    if (ast[t] != ZH_OK) continue;
    const Table& tab = tables[t];
    const size_t n = tab.entries.size();
    zh_zip_reader* r = zh_zip_reader_new(images[t], lens[t]);
    made.r[t] = r;
    std::vector<uint64_t> off(n, 0), len(n, 0);
    std::vector<int32_t> stt(n, ZH_OK);
    std::vector<void*> red(n, nullptr);
    std::vector<uint16_t> dtime(n), ddate(n);
    std::vector<uint8_t> in_dir(n);
    for (size_t i = 0; i < n; i++) {
      const Table::Entry& en = tab.entries[i];
      const ZhZrRec& e = recs[en.rec];
      zh_zip_reader_add(r, en.key, en.directory, (int64_t)e.pos, e.crc, (int64_t)e.csize, (int64_t)e.usize, en.unix_mode);
      off[i] = slots[slot_of[en.rec]].dst - aoff[t];
      len[i] = e.usize;
      dtime[i] = e.dos_time;
      ddate[i] = e.dos_date;
      in_dir[i] = en.in_directory ? 1 : 0;
    }
    void* const block = blocks[t];
    if (block) own.p[blocks_at + t] = nullptr;  // the reader's from here on
    zh_zip_reader_set_data(r, block, (size_t)alen[t], off.data(), len.data(), stt.data(), red.data());
    zh_zip_reader_set_v1(r, dtime.data(), ddate.data(), in_dir.data());
  }
  for (size_t t = 0; t < n_zip; t++) {
    readers[t] = made.r[t];
    statuses[t] = ast[t];
    made.r[t] = nullptr;
  }
  return ZH_OK;
}
