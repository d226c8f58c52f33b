// Reading zip archives: openZipArchive (src/zippy/ziparchives.nim:183-372) and the extraction loop of extractAll
// (:374-453, without the file system) for many images a call.  The host only locates each image's central directory
// (the end records: a few fixed-size reads, zh_zip_locate); all images are uploaded once and stay in HBM as the
// sources of everything that follows:
//   zh_zip_next_kernel    every byte of every directory span is read as if a central record started there: next[b]
//   zh_walk_double_kernel the positions reachable from an archive's first central header ARE its records (zh_walk.h)
//   zh_walk_scan_*        a prefix sum over the marks: every record's ordinal in directory order, the list of records
//   zh_zip_parse_kernel   one wave per record: the checks of openZipArchive's loop body in its order, the name's
//                         UTF-8 validity and safety, the local header's checks of extractFile; one fixed-size record
//   zh_zip_reduce_kernel  per archive: the first record that failed (and later: the first file entry that failed)
//   (host)                readers from the records: paths copied or converted, duplicates found on insertion; the
//                         layout of the output; ONE uncompress plan over every deflated entry of the call, its
//                         sources in place in the uploaded images
//   zh_zip_finish_kernel  stored entries copied image -> slot, every entry's CRC-32 held against its record
//                         (zh_zip_dev.h, with the host stages around it)
// The host parses no central record and no local header, compares no CRC and copies no entry.
//
// Scratch of the walk: 16 bytes per node -- two jump arrays, the marks, the ordinals, 4 bytes each.  A node is a byte
// of [socd, socd + cd_size] clipped to the image, so the walk costs 16 bytes of HBM per directory byte (Bagnon's 300
// records: 24 KiB of directory, 390 KiB of scratch), plus 4 bytes per 1024 nodes for the scan.
//
// The plan reads whole aligned 32-bit words around a source and the stored copy reads aligned 16-byte chunks up to 31
// bytes past a source byte: every image sits at an 8-byte aligned offset of ONE allocation that ends with 512 spare
// bytes, so those reads stay inside it whatever an archive's last byte is.
#include <unordered_set>

#include "zh_walk.h"
#include "zh_zip_dev.h"

namespace {

constexpr uint32_t kLocalSig = 0x04034b50u, kCentralSig = 0x02014b50u;
constexpr uint64_t kRecordMax = 46 + 3 * 65535;  // the longest central record: name, extra and comment of 65535 bytes

// One archive of the walk.  All archives of a call share one index space of nodes: this one's are node0 + k for the
// positions socd + k, k = 0 .. span (span = min(socd + cd_size, len) - socd: a record may START at socd + cd_size --
// it fails there, or at the image's end --, and no more than num_records * kRecordMax: further no record of the
// directory's count can start), followed by its END node node0 + span + 1, which points to itself.
struct ZhZipImg {
  const uint8_t* data;  // device address of the image, 8-byte aligned
  uint64_t len;
  uint64_t up_off;      // ... as an offset into the upload buffer
  uint64_t socd, cd_end;  // the first central header; socd + cd_size
  int64_t socd_offset;
  uint64_t num_records;
  uint32_t node0, span;
};

// One central directory record as openZipArchive keeps it (:275-361), plus what extractFile (:39-93) finds at its
// local header.  status: the first check of the loop body that failed; after_dup: that check comes behind the
// duplicate check (which the host makes when it inserts the path).
struct ZhZipRec {
  uint64_t name_off;             // the raw name is image bytes [name_off, + name_len)
  int64_t header_offset;         // -1: no image can hold it
  int64_t compressed_size, uncompressed_size;
  uint64_t src_off, src_len;     // file records whose local header passed: the stream in the upload buffer
  uint64_t cap;                  // ... and the output capacity
  uint32_t name_len, crc, unix_mode;
  int32_t status, local_status;
  uint16_t local_method;
  uint8_t directory, from_cp437, after_dup, unsafe;
};

__device__ __forceinline__ uint32_t find_img(const ZhZipImg* __restrict__ imgs, uint32_t n_img, uint32_t node) {
  uint32_t lo = 0, hi = n_img;  // the last archive whose node0 <= node
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (imgs[mid].node0 <= node)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

}  // namespace

// next[b] for every node b: the node behind the record if a central record starts at b's position -- END when the 46
// bytes are not inside the image, when the signature is another, when the record ends behind the span, and for END
// itself.  mark[b] = 1 for the first position of every archive that has records.
__global__ __launch_bounds__(256) void zh_zip_next_kernel(const ZhZipImg* __restrict__ imgs, uint32_t n_img,
                                                          uint32_t n_nodes, uint32_t* __restrict__ jump,
                                                          uint32_t* __restrict__ mark) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n_nodes) return;
  const ZhZipImg g = imgs[find_img(imgs, n_img, b)];
  const uint32_t end = g.node0 + g.span + 1;
  uint32_t nx = end;
  if (b != end) {
    const uint64_t pos = g.socd + (b - g.node0);
    const uint8_t* __restrict__ p = g.data + pos;
    if (pos + 46 <= g.len && p[0] == 0x50 && ld32(p) == kCentralSig) {
      const uint64_t k = (uint64_t)(b - g.node0) + 46 + ld16(p + 28) + ld16(p + 30) + ld16(p + 32);
      if (k <= g.span) nx = g.node0 + (uint32_t)k;
    }
  }
  jump[b] = nx;
  mark[b] = b == g.node0 && g.num_records != 0 ? 1u : 0u;
}

// One wave per record, in directory order (h = its ordinal in the call, list[h] its node).  The fields are read by
// every lane (the same addresses: one broadcast load each); the name's bytes go over the lanes.  The checks follow
// openZipArchive's loop body (:275-361): the 46 bytes are there, the signature, the method, the file's disk, the name
// is inside the image -- [here the host checks for a duplicate] -- the zip64 extra, the directory's size; sizes and
// offsets that no image can hold become -1 as in zh_zip_open.  Records behind the archive's count are not looked at.
// A file record then gets extractFile's checks of its local header (:54-72, in zh_zip_extract_batch's order).
__global__ __launch_bounds__(256) void zh_zip_parse_kernel(const ZhZipImg* __restrict__ imgs, uint32_t n_img,
                                                           const uint32_t* __restrict__ ord,
                                                           const uint32_t* __restrict__ list, uint32_t n_rec,
                                                           ZhZipRec* __restrict__ recs, int32_t* __restrict__ rstat,
                                                           uint8_t* __restrict__ runsafe) {
  const uint32_t h = blockIdx.x * 4 + (threadIdx.x >> 6), lane = zh_lane();
  if (h >= n_rec) return;
  const uint32_t node = list[h];
  const ZhZipImg g = imgs[find_img(imgs, n_img, node)];
  const int64_t size = (int64_t)g.len;
  ZhZipRec rec{};
  int32_t status = ZH_OK;
  bool after_dup = false, unsafe = false;
  if ((uint64_t)(h - ord[g.node0]) < g.num_records) {
    int64_t pos = (int64_t)(g.socd + (node - g.node0));
    const uint8_t* __restrict__ p = g.data + pos;
    if (!has(size, pos, 46)) {
      status = ZH_ERR_ARCHIVE_EOF;
    } else if (ld32(p) != kCentralSig) {
      status = ZH_ERR_ZIP_CENTRAL_HEADER;
    } else {
      const uint32_t flags = ld16(p + 8), method = ld16(p + 10), crc = ld32(p + 16);
      const int64_t name_len = ld16(p + 28), extra_len = ld16(p + 30), comment_len = ld16(p + 32);
      const uint32_t file_disk = ld16(p + 34), external = ld32(p + 38);
      int64_t csize = ld32(p + 20), usize = ld32(p + 24), hoff = ld32(p + 42);
      pos += 46;
      if (method != 0 && method != 8) {
        status = ZH_ERR_ZIP_METHOD;
      } else if (file_disk != 0) {
        status = ZH_ERR_ZIP_DISK_NUMBER;
      } else if (!has(size, pos, name_len)) {
        status = ZH_ERR_ARCHIVE_EOF;
      } else {
        const uint8_t* __restrict__ q = g.data + pos;
        rec.name_off = (uint64_t)pos;
        rec.name_len = (uint32_t)name_len;
        // validate_utf8's rule (zh_zip.hip), a position a lane: no byte that cannot lead, every lead followed by
        // exactly its continuation bytes, no continuation byte in front; and the path rule at every position
        bool bad = false, risky = false;
        for (int64_t j = lane; j < name_len; j += 64) {
          uint32_t c[5];
#pragma unroll
          for (int k = 0; k < 5; k++) c[k] = j + k < name_len ? q[j + k] : 0u;
          const bool tail[5] = {false, j + 1 < name_len && (c[1] >> 6) == 2, j + 2 < name_len && (c[2] >> 6) == 2,
                                j + 3 < name_len && (c[3] >> 6) == 2, j + 4 < name_len && (c[4] >> 6) == 2};
          const uint32_t c0 = c[0];
          if (c0 <= 127) {
            bad = bad || tail[1];
          } else if ((c0 >> 5) == 6) {
            bad = bad || c0 < 0xc2 || !tail[1] || tail[2];
          } else if ((c0 >> 4) == 14) {
            bad = bad || !tail[1] || !tail[2] || tail[3];
          } else if ((c0 >> 3) == 30) {
            bad = bad || !tail[1] || !tail[2] || !tail[3] || tail[4];
          } else if ((c0 >> 6) == 2) {
            bad = bad || j == 0;  // (elsewhere the byte in front answers for it)
          } else {
            bad = true;
          }
          // (the path rule looks at ASCII bytes only, and utf8ify (ziparchives.nim:108-160) keeps every ASCII byte and
          // turns a byte >= 0x80 into bytes >= 0x80: the raw name is unsafe exactly when the converted path is)
          risky = risky || unsafe_at(c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24), (uint64_t)j);
        }
        const bool invalid_utf8 = __ballot(bad) != 0;
        unsafe = __ballot(risky) != 0;
        rec.from_cp437 = !(flags & 0x0800u) && invalid_utf8 ? 1 : 0;
        pos += name_len;
        // :303-341 the zip64 sizes; the field header is read at the FIRST extra field, as the reference reads it
        if (extra_len > 0) {
          if (!has(size, pos, 4)) {
            status = ZH_ERR_ARCHIVE_EOF;
          } else if (ld16(g.data + pos) == 1) {
            int64_t at = pos + 4;
            const int64_t fend = at + (int64_t)ld16(g.data + pos + 2);
            int64_t* const fields[3] = {&usize, &csize, &hoff};
#pragma unroll
            for (int k = 0; k < 3; k++) {
              if (status != ZH_OK || *fields[k] != 0xffffffffll) continue;
              if (at > fend - 8 || !has(size, at, 8)) {
                status = ZH_ERR_ARCHIVE_EOF;
              } else {
                *fields[k] = (int64_t)ld64(g.data + at);
                at += 8;
              }
            }
          }
        }
        pos += extra_len + comment_len;
        if (status == ZH_OK && (uint64_t)pos > g.cd_end) status = ZH_ERR_ZIP_CENTRAL_SIZE;
        after_dup = status != ZH_OK;
        if (hoff < 0 || hoff > size) hoff = -1;
        if (csize < 0 || csize > size) csize = -1;
        if (usize < 0) usize = -1;
        rec.directory = (external & 0x10u) != 0 || (external & (0x4000u << 16)) != 0 ||
                        (name_len > 0 && q[name_len - 1] == '/');
        rec.header_offset = hoff < 0 ? -1 : hoff + g.socd_offset;
        rec.crc = crc;
        rec.compressed_size = csize;
        rec.uncompressed_size = usize;
        rec.unix_mode = external >> 16;
        if (status == ZH_OK && !rec.directory) {  // extractFile's local header
          int64_t lp = rec.header_offset;
          if (!has(size, lp, 30)) {
            rec.local_status = ZH_ERR_ARCHIVE_EOF;
          } else if (ld32(g.data + lp) != kLocalSig) {
            rec.local_status = ZH_ERR_ZIP_FILE_HEADER;
          } else {
            const uint32_t lmethod = ld16(g.data + lp + 8);  // the LOCAL header's method decides (:62)
            lp += 30 + (int64_t)ld16(g.data + lp + 26) + (int64_t)ld16(g.data + lp + 28);
            if (usize < 0 || !has(size, lp, csize)) {
              rec.local_status = ZH_ERR_ARCHIVE_EOF;
            } else if (lmethod != 0 && lmethod != 8) {
              rec.local_status = ZH_ERR_ZIP_METHOD;
            } else {
              rec.local_method = (uint16_t)lmethod;
              rec.src_off = g.up_off + (uint64_t)lp;
              rec.src_len = (uint64_t)csize;
              // (deflate cannot expand beyond 1032:1; a size above that is a damaged directory)
              const uint64_t bound = (uint64_t)csize * 1032 + 1024;
              rec.cap = lmethod == 0 ? (uint64_t)csize : ((uint64_t)usize < bound ? (uint64_t)usize : bound);
            }
          }
        }
      }
    }
  }
  rec.status = status;
  rec.after_dup = after_dup ? 1 : 0;
  rec.unsafe = unsafe ? 1 : 0;
  if (lane == 0) {
    recs[h] = rec;
    rstat[h] = status;
    runsafe[h] = unsafe ? 1 : 0;
  }
}

// The archives' ranges of records for the reduction: [ord[node0], + min(records on the chain, num_records))
__global__ __launch_bounds__(256) void zh_zip_ranges_kernel(const ZhZipImg* __restrict__ imgs, uint32_t n_img,
                                                            const uint32_t* __restrict__ ord,
                                                            uint32_t* __restrict__ ranges) {
  const uint32_t a = blockIdx.x * 256 + threadIdx.x;
  if (a >= n_img) return;
  const ZhZipImg g = imgs[a];
  const uint32_t first = ord[g.node0], found = ord[g.node0 + g.span + 1] - first;
  ranges[2 * a] = first;
  ranges[2 * a + 1] = first + (uint32_t)((uint64_t)found < g.num_records ? (uint64_t)found : g.num_records);
}

extern "C" int zh_zip_open_all_batch(zh_ctx* ctx, const void* const* images, const size_t* lens, size_t n_zip,
                                     zh_zip_reader** readers, int32_t* statuses) {
  if (const int e = reader_checks(ctx, images, lens, n_zip, readers, statuses)) return e;
  if (!n_zip) return ZH_OK;

  // ---- 1. the directories (host: the end records only) ----
  std::vector<size_t> walk;  // the archives that go on
  std::vector<ZhZipImg> imgs;
  std::vector<const void*> up_src;
  std::vector<uint64_t> up_off, up_len;
  uint64_t up_total = 0, n_nodes = 0, max_chain = 0, sum_records = 0;
  for (size_t t = 0; t < n_zip; t++) {
    ZhZipDirectory dir;
    if ((statuses[t] = zh_zip_locate(images[t], lens[t], &dir)) != ZH_OK) continue;
    ZhZipImg g{};
    g.len = lens[t];
    g.up_off = up_total;
    g.socd = (uint64_t)dir.socd;
    g.cd_end = (uint64_t)(dir.socd + dir.cd_size);
    g.socd_offset = dir.socd - dir.cd_start;
    g.num_records = (uint64_t)dir.num_records;
    // cd_size is the (untrusted) end record's word: the nodes end where the chain of num_records records can reach
    // at the latest -- record k starts no further than k * kRecordMax behind socd --, so that an end record that
    // claims the whole image as its directory costs scratch by its record count, not by the image
    const uint64_t reach = g.num_records > ~0ull / kRecordMax ? ~0ull : g.num_records * kRecordMax;
    const uint64_t span = std::min<uint64_t>(std::min<uint64_t>(g.cd_end, g.len) - g.socd, reach);
    sum_records += g.num_records;
    if (n_nodes + span + 2 >= 0xffffffffull || sum_records >= 0xffffffffull) return ZH_ERR_ARGUMENT;
    g.node0 = (uint32_t)n_nodes;
    g.span = (uint32_t)span;
    n_nodes += span + 2;
    max_chain = std::max(max_chain, std::min<uint64_t>(g.num_records, span / 46 + 1));
    walk.push_back(t);
    imgs.push_back(g);
    up_src.push_back(images[t]);
    up_off.push_back(up_total);
    up_len.push_back(lens[t]);
    up_total += round_up8(lens[t]);
  }
  const size_t n_walk = walk.size();
  if (!n_walk) return ZH_OK;
  ZH_HIP(ctx, hipSetDevice(ctx->device));
  Trace tr;
  int st;
  hipStream_t s = ctx->stream;
  const dim3 wg(256);

  // ---- 2. one upload ----
  DevBuf d_in;
  if (dev_alloc(ctx, d_in, up_total + 512) != hipSuccess) return ZH_ERR_NOMEM;
  if ((st = zhh_upload_slices(ctx, up_src.data(), up_off, up_len, up_total, d_in.p))) return st;
  for (size_t k = 0; k < n_walk; k++) imgs[k].data = d_in.p + imgs[k].up_off;
  tr.mark(ctx, "zip open: upload");

  // ---- 3. the walk ----
  // after `rounds` rounds every node up to 2^rounds - 1 steps from a start is marked; max_chain records are wanted
  uint32_t rounds = 0;
  while ((1ull << rounds) < max_chain + 1) rounds++;
  const uint32_t N = (uint32_t)n_nodes;
  DevBuf d_imgs;
  std::vector<uint64_t> ioff;
  if ((st = zhh_upload_spans(ctx, {{imgs.data(), n_walk * sizeof(ZhZipImg)}}, d_imgs, ioff))) return st;
  Walk w;
  if ((st = walk_alloc(ctx, w, N))) return st;
  // (plain pointers for the launches: a launch must not take a DevBuf, or the Walk that holds one, along)
  const ZhZipImg* const dimgs = reinterpret_cast<const ZhZipImg*>(d_imgs.p);
  uint32_t *const j0 = w.j0, *const mark = w.mark;
  const uint32_t *const ord = w.ord, *const list = w.list;
  Events evs;  // ZH_TRACE: the walk's kernels by themselves
  if (tr.on) evs.create();
  if (evs.ok) (void)hipEventRecord(evs.e[0], s);
  hipLaunchKernelGGL(zh_zip_next_kernel, dim3((N + 255) / 256), wg, 0, s, dimgs, (uint32_t)n_walk, N, j0, mark);
  walk_double(w, rounds, s);
  walk_scan(w, s);
  if (evs.ok) (void)hipEventRecord(evs.e[1], s);
  uint32_t n_rec = 0;
  if ((st = walk_count(ctx, w, &n_rec))) return st;
  if (evs.ok) {
    const float ms = evs.ms(0, 1);
    if (ms >= 0)
      fprintf(stderr, "[zh] %-28s %8.3f ms (HIP events; %u nodes, %u rounds)\n", "zip open: walk kernels", ms, N, rounds);
  }
  tr.mark(ctx, "zip open: reach + scan");

  // ---- 4. the records ----
  ZhZipRec* d_recs;
  uint32_t *d_ranges, *d_bad, *d_unsafe;
  int32_t* d_rstat;
  uint8_t* d_rflag;
  Arena out;
  out.add(d_recs, n_rec);
  out.add(d_ranges, n_walk * 2);
  out.add(d_bad, n_walk);
  out.add(d_unsafe, n_walk);
  const size_t out_bytes = out.size;  // (what comes back: the arrays so far)
  out.add(d_rstat, n_rec);
  out.add(d_rflag, n_rec);
  DevBuf d_rec;
  if (out.alloc(ctx, d_rec, 256) != hipSuccess) return ZH_ERR_NOMEM;
  out.bind();
  if (n_rec)
    hipLaunchKernelGGL(zh_zip_parse_kernel, dim3((n_rec + 3) / 4), wg, 0, s, dimgs, (uint32_t)n_walk,
                       ord, list, n_rec, d_recs, d_rstat, d_rflag);
  hipLaunchKernelGGL(zh_zip_ranges_kernel, dim3(((uint32_t)n_walk + 255) / 256), wg, 0, s, dimgs, (uint32_t)n_walk,
                     ord, d_ranges);
  hipLaunchKernelGGL(zh_zip_reduce_kernel, dim3((uint32_t)n_walk), wg, 0, s, (const uint32_t*)d_ranges,
                     (const int32_t*)d_rstat, (const uint8_t*)d_rflag, d_bad, d_unsafe);
  ZH_HIP(ctx, hipGetLastError());
  HostBufs own;
  void* h_rec = nullptr;
  {
    size_t got = 0;
    int32_t dst_st = ZH_OK;
    st = zhh_download(ctx, d_rec.p, 1, {0}, {out_bytes}, {1}, &h_rec, &got, &dst_st);
    own.p.push_back(h_rec);
    if (st || dst_st) return st ? st : dst_st;
  }
  const ZhZipRec* const recs = out.host(h_rec, d_recs);
  const uint32_t* const ranges = out.host(h_rec, d_ranges);
  const uint32_t* const first_bad = out.host(h_rec, d_bad);
  const uint32_t* const any_unsafe = out.host(h_rec, d_unsafe);
  tr.mark(ctx, "zip open: parse + reduce");

  // ---- 5. the readers, from the records: string building, the duplicate check, the serial loop's precedence ----
  Readers made;
  made.r.assign(n_walk, nullptr);
  std::vector<int32_t> ast(n_walk, ZH_OK);
  std::vector<ZipSlot> slots;  // the file entries of the archives that are extracted
  std::vector<uint32_t> eranges(2 * n_walk, 0);  // an archive's slots are contiguous
  std::vector<uint64_t> aoff(n_walk, 0), alen(n_walk, 0);
  uint64_t out_total = 0;
  for (size_t k = 0; k < n_walk; k++) {
    const uint8_t* const image = (const uint8_t*)images[walk[k]];
    const uint32_t lo = ranges[2 * k], hi = ranges[2 * k + 1];
    // records behind the first that failed on the device are never reached by the serial loop
    const uint32_t stop = first_bad[k] == kNone ? hi : first_bad[k] + 1;
    zh_zip_reader* r = zh_zip_reader_new(image, lens[walk[k]]);
    std::unordered_set<std::string> seen;
    int status = ZH_OK;
    for (uint32_t i = lo; i < stop && status == ZH_OK; i++) {
      const ZhZipRec& e = recs[i];
      if (e.status != ZH_OK && !e.after_dup) {
        status = e.status;
        break;
      }
      std::string raw((const char*)image + e.name_off, e.name_len);
      if (seen.count(raw)) {  // zh_zip_open's rule: the raw name against the paths kept so far
        status = ZH_ERR_ZIP_DUPLICATE;
        break;
      }
      if (e.status != ZH_OK) {
        status = e.status;
        break;
      }
      std::string path = e.from_cp437 ? zh_zip_from_cp437(raw.data(), raw.size()) : std::move(raw);
      seen.insert(path);
      zh_zip_reader_add(r, std::move(path), e.directory != 0, e.header_offset, e.crc, e.compressed_size,
                        e.uncompressed_size, e.unix_mode);
    }
    // a chain that ends before the directory's count: the next record would start behind the image
    if (status == ZH_OK && (uint64_t)(hi - lo) < imgs[k].num_records) status = ZH_ERR_ARCHIVE_EOF;
    if (status != ZH_OK) {
      zh_zip_close(r);
      ast[k] = status;
      continue;
    }
    made.r[k] = r;
    if (any_unsafe[k]) {  // extractAll checks every path before it extracts anything (:417-419)
      ast[k] = ZH_ERR_UNSAFE_PATH;
      continue;
    }
    out_total = (out_total + 15) & ~(uint64_t)15;  // (the download moves a block 16 bytes at a time)
    aoff[k] = out_total;
    eranges[2 * k] = (uint32_t)slots.size();
    for (uint32_t i = lo; i < hi; i++) {
      const ZhZipRec& e = recs[i];
      if (e.directory) continue;
      ZipSlot sl{k, i, e.src_off, e.src_len, 0, 0, e.crc, 0, e.local_status, e.local_method};
      if (e.local_status == ZH_OK) {
        // (what zh_uncompress_batch_sized makes of zh_zip_extract_batch's hint: never above its expansion bound)
        sl.cap = e.local_method == 8 ? std::min<uint64_t>(e.cap, e.src_len * 1032 + 64) : e.cap;
        sl.dst = out_total;
        out_total += round_up8(sl.cap);
      }
      slots.push_back(sl);
    }
    eranges[2 * k + 1] = (uint32_t)slots.size();
    alen[k] = out_total - aoff[k];
  }
  const size_t n_slot = slots.size();
  if (n_slot >= 0xffffffffull) return ZH_ERR_ARGUMENT;
  tr.mark(ctx, "zip open: readers");

  // ---- 6. one decode; 7. the stored entries and every verdict; 8. one download: every archive's block ----
  std::vector<int32_t> est;
  std::vector<uint64_t> elen;
  std::vector<uint32_t> ebad(n_walk, kNone);
  std::vector<void*> blocks(n_walk, nullptr);
  size_t blocks_at = 0;
  if (n_slot) {
    DevBuf d_out;
    if ((st = zip_extract(ctx, tr, "zip open", slots, eranges, d_in.p, out_total, false, d_out, est, &elen, ebad)))
      return st;
    std::vector<char> take(n_walk, 0);
    for (size_t k = 0; k < n_walk; k++) take[k] = made.r[k] && ast[k] == ZH_OK && alen[k] ? 1 : 0;
    if ((st = zip_download(ctx, d_out.p, aoff, alen, take, own, blocks, &blocks_at))) return st;
    tr.mark(ctx, "zip open: download");
  }

  // An entry that outgrew its slot has a directory that understates its size; the reference does not look at the
  // size field, only at the CRC: such an entry is decoded again (zip_redo), and a reader keeps the result.
  std::vector<void*> redone(n_slot, nullptr);
  if ((st = zip_redo(ctx, tr, "zip open", slots, eranges, up_src.data(), up_off, own, est, ebad,
                     [&](size_t j, int32_t rst, uint32_t rcrc, size_t rout, void*& buf) {
                       const int32_t v = rst == ZH_OK && rcrc != slots[j].want_crc ? ZH_ERR_ZIP_CRC : rst;
                       elen[j] = v == ZH_OK ? rout : 0;
                       if (v == ZH_OK) {  // the reader's from here on
                         redone[j] = buf;
                         buf = nullptr;
                       }
                       return v;
                     })))
    return st;

  // ---- the results into the readers ----
  {
    size_t j = 0;
    for (size_t k = 0; k < n_walk; k++) {
      zh_zip_reader* r = made.r[k];
      if (!r) continue;
      const size_t n = zh_zip_num_entries(r);
      std::vector<uint64_t> off(n, 0), len(n, 0);
      std::vector<int32_t> stt(n, ZH_OK);
      std::vector<void*> red(n, nullptr);
      if (ast[k] == ZH_ERR_UNSAFE_PATH) {  // nothing was extracted: a file entry says why
        const uint32_t lo = ranges[2 * k];
        for (size_t i = 0; i < n; i++)
          if (!recs[lo + i].directory) stt[i] = ZH_ERR_UNSAFE_PATH;
      } else {
        for (; j < n_slot && slots[j].img == k; j++) {
          const size_t i = slots[j].rec - ranges[2 * k];
          off[i] = slots[j].dst - aoff[k];
          len[i] = elen[j];
          stt[i] = est[j];
          red[i] = redone[j];
        }
        if (ebad[k] != kNone) ast[k] = est[ebad[k]];
      }
      void* const block = blocks[k];
      if (block) own.p[blocks_at + k] = nullptr;  // the reader's from here on
      zh_zip_reader_set_data(r, block, (size_t)alen[k], off.data(), len.data(), stt.data(), red.data());
    }
  }
  for (size_t k = 0; k < n_walk; k++) {
    readers[walk[k]] = made.r[k];
    statuses[walk[k]] = ast[k];
    made.r[k] = nullptr;
  }
  return ZH_OK;
}
