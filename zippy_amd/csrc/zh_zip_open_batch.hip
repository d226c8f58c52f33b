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

#include "zh_host.h"
#include "zh_gather.h"
#include "zh_walk.h"
#include "zh_zip_dev.h"

namespace {

constexpr uint32_t kLocalSig = 0x04034b50u, kCentralSig = 0x02014b50u;
constexpr uint64_t kSlice = 32768;  // bytes of a stored entry a wave copies at most
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

// One file entry of an archive that opened, for zh_zip_finish_kernel
struct ZhZipFin {
  uint64_t src, dst, len;  // a stored entry: len bytes from upload buffer + src to output buffer + dst
  uint32_t want_crc;
  int32_t local_status;    // not ZH_OK: nothing to extract, this is the entry's status
  uint32_t deflated;       // 1: result `idx` of the plan; 0: stored entry `idx` of the checksum launch
  uint32_t idx;
};
struct ZhZipFinTask {
  uint64_t lo, hi;  // bytes [lo, hi) of the entry's data
  uint32_t entry, first;
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

// internal.nim:294-302 verifyPathIsSafeToExtract on the four bytes x of a path that start at position `at`.  The
// rule looks at ASCII bytes only, and utf8ify (ziparchives.nim:108-160) keeps every ASCII byte and turns a byte
// >= 0x80 into bytes >= 0x80: the raw name is unsafe exactly when the converted path is, so the raw name is checked.
// (The same rule as zh_tar_open_batch.hip's.)
__device__ __forceinline__ bool unsafe_at(uint32_t x, uint64_t at) {
  if (x == 0x2f2e2e2fu || x == 0x5c2e2e5cu) return true;  // "/../", "\..\"
  if (at != 0) return false;
  return (x & 0xffu) == '/' || (x & 0xffffffu) == 0x2f2e2eu || (x & 0xffffffu) == 0x5c2e2eu;  // "/", "../", "..\"
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

// One wave per task (four a workgroup): a slice of a stored entry's bytes goes from its image to its slot -- the
// bytes in front of the first and behind the last aligned 16-byte chunk of the slot one a lane, the chunks in between
// with one 16-byte store each, their bytes gathered from the (differently aligned) source.  The wave of an entry's
// first task also settles the entry: a local header that failed, else the decoder's status (deflated entries: the
// plan's status, length and CRC-32), else the CRC-32 against the record's (:91-92).
__global__ __launch_bounds__(256) void zh_zip_finish_kernel(const uint8_t* __restrict__ d_in, uint8_t* __restrict__ d_out,
                                                            const ZhZipFin* __restrict__ fins,
                                                            const ZhZipFinTask* __restrict__ tasks, uint32_t n_tasks,
                                                            const int32_t* __restrict__ plan_st,
                                                            const uint64_t* __restrict__ plan_len,
                                                            const uint32_t* __restrict__ plan_crc,
                                                            const uint32_t* __restrict__ stored_crc,
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
      if (st != ZH_OK) len = 0;
    }
    est[t.entry] = st;
    elen[t.entry] = len;
  }
  if (t.lo >= t.hi) return;
  const uint64_t a = e.dst + t.lo, b = e.dst + t.hi, delta = e.src - e.dst;  // (source byte = slot byte + delta, mod 2^64)
  const uint64_t A = (a + 15) & ~(uint64_t)15, B = b & ~(uint64_t)15;
  if (A >= B) {  // no whole chunk inside: at most 30 bytes
    if (a + lane < b) d_out[a + lane] = d_in[a + lane + delta];
    return;
  }
  if (a + lane < A) d_out[a + lane] = d_in[a + lane + delta];
  if (B + lane < b) d_out[B + lane] = d_in[B + lane + delta];
  for (uint64_t c = A + 16ull * lane; c < B; c += 1024) *reinterpret_cast<Chunk16*>(d_out + c) = gather16(d_in, c + delta);
}

extern "C" int zh_zip_open_all_batch(zh_ctx* ctx, const void* const* images, const size_t* lens, size_t n_zip,
                                     zh_zip_reader** readers, int32_t* statuses) {
  if (!ctx || (n_zip && (!images || !lens || !readers || !statuses))) return ZH_ERR_ARGUMENT;
  for (size_t t = 0; t < n_zip; t++) {
    readers[t] = nullptr;
    statuses[t] = ZH_OK;
  }
  for (size_t t = 0; t < n_zip; t++)
    if (!images[t] && lens[t]) return ZH_ERR_ARGUMENT;
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
  const uint32_t N = (uint32_t)n_nodes, n_sums = (N + kScanItems - 1) / kScanItems;
  DevBuf d_imgs, d_scr;
  std::vector<uint64_t> ioff;
  if ((st = zhh_upload_spans(ctx, {{imgs.data(), n_walk * sizeof(ZhZipImg)}}, d_imgs, ioff))) return st;
  Arena ar;
  const size_t o_j0 = ar.reserve((size_t)N * 4), o_j1 = ar.reserve((size_t)N * 4), o_mark = ar.reserve((size_t)N * 4),
               o_ord = ar.reserve((size_t)N * 4), o_sums = ar.reserve(((size_t)n_sums + 1) * 4);
  if (dev_alloc(ctx, d_scr, ar.size) != hipSuccess) return ZH_ERR_NOMEM;
  uint32_t* const j0 = carve<uint32_t>(d_scr.p, o_j0);
  uint32_t* const j1 = carve<uint32_t>(d_scr.p, o_j1);
  uint32_t* const mark = carve<uint32_t>(d_scr.p, o_mark);
  uint32_t* const ord = carve<uint32_t>(d_scr.p, o_ord);
  uint32_t* const sums = carve<uint32_t>(d_scr.p, o_sums);
  const ZhZipImg* const dimgs = reinterpret_cast<const ZhZipImg*>(d_imgs.p);
  const dim3 node_grid((N + 255) / 256);
  struct Events {  // ZH_TRACE: the walk's kernels by themselves, between two events that go away with the scope
    hipEvent_t e[2] = {nullptr, nullptr};
    bool ok = false;
    ~Events() {
      for (hipEvent_t x : e)
        if (x) (void)hipEventDestroy(x);
    }
  } evs;
  if (tr.on) evs.ok = hipEventCreate(&evs.e[0]) == hipSuccess && hipEventCreate(&evs.e[1]) == hipSuccess;
  hipEvent_t* const ev = evs.e;
  if (evs.ok) (void)hipEventRecord(ev[0], s);
  hipLaunchKernelGGL(zh_zip_next_kernel, node_grid, wg, 0, s, dimgs, (uint32_t)n_walk, N, j0, mark);
  uint32_t *jin = j0, *jout = j1;
  for (uint32_t r = 0; r < rounds; r++) {
    hipLaunchKernelGGL(zh_walk_double_kernel, node_grid, wg, 0, s, (const uint32_t*)jin, jout, mark, N);
    std::swap(jin, jout);
  }
  // (the jump arrays are dead from here on: the list of records takes the place of the first)
  uint32_t* const list = j0;
  hipLaunchKernelGGL(zh_walk_scan_sums_kernel, dim3(n_sums), wg, 0, s, (const uint32_t*)mark, N, sums);
  hipLaunchKernelGGL(zh_walk_scan_offsets_kernel, dim3(1), wg, 0, s, sums, n_sums);
  hipLaunchKernelGGL(zh_walk_scan_write_kernel, dim3(n_sums), wg, 0, s, (const uint32_t*)mark, N,
                     (const uint32_t*)sums, ord, list);
  if (evs.ok) (void)hipEventRecord(ev[1], s);
  ZH_HIP(ctx, hipGetLastError());
  uint32_t n_rec = 0;  // the records are sized by the marks there are, not by the nodes
  ZH_HIP(ctx, hipMemcpyAsync(&n_rec, sums + n_sums, 4, hipMemcpyDeviceToHost, s));
  ZH_HIP(ctx, hipStreamSynchronize(s));
  if (evs.ok) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess)
      fprintf(stderr, "[zh] %-28s %8.3f ms (HIP events; %u nodes, %u rounds)\n", "zip open: walk kernels", ms, N, rounds);
  }
  tr.mark(ctx, "zip open: reach + scan");

  // ---- 4. the records ----
  Arena out;
  const size_t o_recs = out.reserve((size_t)n_rec * sizeof(ZhZipRec)), o_ranges = out.reserve(n_walk * 8),
               o_bad = out.reserve(n_walk * 4), o_unsafe = out.reserve(n_walk * 4);
  const size_t out_bytes = out.size;
  const size_t o_rstat = out.reserve((size_t)n_rec * 4), o_rflag = out.reserve((size_t)n_rec);
  DevBuf d_rec;
  if (dev_alloc(ctx, d_rec, out.size + 256) != hipSuccess) return ZH_ERR_NOMEM;
  if (n_rec)
    hipLaunchKernelGGL(zh_zip_parse_kernel, dim3((n_rec + 3) / 4), wg, 0, s, dimgs, (uint32_t)n_walk,
                       (const uint32_t*)ord, (const uint32_t*)list, n_rec, carve<ZhZipRec>(d_rec.p, o_recs),
                       carve<int32_t>(d_rec.p, o_rstat), carve<uint8_t>(d_rec.p, o_rflag));
  hipLaunchKernelGGL(zh_zip_ranges_kernel, dim3(((uint32_t)n_walk + 255) / 256), wg, 0, s, dimgs, (uint32_t)n_walk,
                     (const uint32_t*)ord, carve<uint32_t>(d_rec.p, o_ranges));
  hipLaunchKernelGGL(zh_zip_reduce_kernel, dim3((uint32_t)n_walk), wg, 0, s,
                     (const uint32_t*)carve<uint32_t>(d_rec.p, o_ranges), (const int32_t*)carve<int32_t>(d_rec.p, o_rstat),
                     (const uint8_t*)carve<uint8_t>(d_rec.p, o_rflag), carve<uint32_t>(d_rec.p, o_bad),
                     carve<uint32_t>(d_rec.p, o_unsafe));
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
  const uint8_t* const hr = (const uint8_t*)h_rec;
  const ZhZipRec* const recs = reinterpret_cast<const ZhZipRec*>(hr + o_recs);
  const uint32_t* const ranges = reinterpret_cast<const uint32_t*>(hr + o_ranges);
  const uint32_t* const first_bad = reinterpret_cast<const uint32_t*>(hr + o_bad);
  const uint32_t* const any_unsafe = reinterpret_cast<const uint32_t*>(hr + o_unsafe);
  tr.mark(ctx, "zip open: parse + reduce");

  // ---- 5. the readers, from the records: string building, the duplicate check, the serial loop's precedence ----
  Readers made;
  made.r.assign(n_walk, nullptr);
  std::vector<int32_t> ast(n_walk, ZH_OK);
  struct Slot {  // a file entry of an archive that is extracted
    size_t walk, entry;
    const ZhZipRec* rec;
    uint64_t dst = 0, cap = 0;
  };
  std::vector<Slot> slots;
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
    for (uint32_t i = lo; i < hi; i++) {
      const ZhZipRec& e = recs[i];
      if (e.directory) continue;
      Slot sl{k, (size_t)(i - lo), &e};
      if (e.local_status == ZH_OK) {
        // (what zh_uncompress_batch_sized makes of zh_zip_extract_batch's hint: never above its expansion bound)
        sl.cap = e.local_method == 8 ? std::min<uint64_t>(e.cap, e.src_len * 1032 + 64) : e.cap;
        sl.dst = out_total;
        out_total += round_up8(sl.cap);
      }
      slots.push_back(sl);
    }
    alen[k] = out_total - aoff[k];
  }
  const size_t n_slot = slots.size();
  std::vector<size_t> slot_lo(n_walk, 0), slot_hi(n_walk, 0);  // an archive's slots are contiguous
  for (size_t j = 0; j < n_slot; j++) {
    if (!j || slots[j - 1].walk != slots[j].walk) slot_lo[slots[j].walk] = j;
    slot_hi[slots[j].walk] = j + 1;
  }
  if (n_slot >= 0xffffffffull) return ZH_ERR_ARGUMENT;
  tr.mark(ctx, "zip open: readers");

  // ---- 6. one decode; 7. the stored entries and every verdict ----
  std::vector<int32_t> est(n_slot, ZH_OK);
  std::vector<uint64_t> elen(n_slot, 0);
  std::vector<uint32_t> ebad(n_walk, kNone);
  std::vector<void*> blocks(n_walk, nullptr);
  size_t blocks_at = 0;  // blocks[k] is own.p[blocks_at + k] until a reader takes it
  if (n_slot) {
    std::vector<ZhZipFin> fins(n_slot);
    std::vector<ZhZipFinTask> tasks;
    std::vector<uint64_t> p_soff, p_slen, p_doff, p_dcap;
    std::vector<ZhPieceDesc> pieces;
    std::vector<ZhBufDesc> sbufs;
    std::vector<uint32_t> eranges(2 * n_walk, 0);
    for (size_t j = 0; j < n_slot; j++) {
      const Slot& sl = slots[j];
      const ZhZipRec& e = *sl.rec;
      if (!j || slots[j - 1].walk != sl.walk) eranges[2 * sl.walk] = (uint32_t)j;
      eranges[2 * sl.walk + 1] = (uint32_t)j + 1;
      ZhZipFin& f = fins[j];
      f = ZhZipFin{e.src_off, sl.dst, 0, e.crc, e.local_status, 0, 0};
      uint64_t copy = 0;
      if (e.local_status == ZH_OK && e.local_method == 8) {
        f.deflated = 1;
        f.idx = (uint32_t)p_soff.size();
        p_soff.push_back(e.src_off);
        p_slen.push_back(e.src_len);
        p_doff.push_back(sl.dst);
        p_dcap.push_back(sl.cap);
      } else if (e.local_status == ZH_OK) {
        f.len = copy = e.src_len;
        f.idx = (uint32_t)sbufs.size();
        ZhBufDesc b;
        memset(&b, 0, sizeof(b));
        b.src_off = e.src_off;
        b.src_len = copy;
        b.first_piece = (uint32_t)pieces.size();
        for (uint64_t o = 0; o < copy; o += ZH_FRAG_SIZE)
          pieces.push_back(ZhPieceDesc{e.src_off + o, (uint32_t)std::min<uint64_t>(copy - o, ZH_FRAG_SIZE), f.idx, o});
        b.npieces = (uint32_t)pieces.size() - b.first_piece;
        sbufs.push_back(b);
      }
      uint32_t first = 1;
      for (uint64_t o = 0; first || o < copy; o += kSlice, first = 0)
        tasks.push_back(ZhZipFinTask{o, std::min<uint64_t>(copy, o + kSlice), (uint32_t)j, first});
    }
    const size_t n_def = p_soff.size(), n_sto = sbufs.size(), n_piece = pieces.size(), n_task = tasks.size();
    if (n_task >= 0xffffffffull || n_piece >= 0xffffffffull) return ZH_ERR_ARGUMENT;
    DevBuf d_out, d_fin;
    if (dev_alloc(ctx, d_out, out_total + 256) != hipSuccess) return ZH_ERR_NOMEM;
    Arena fa;
    const size_t o_fins = fa.reserve(n_slot * sizeof(ZhZipFin)), o_tasks = fa.reserve(n_task * sizeof(ZhZipFinTask)),
                 o_sbufs = fa.reserve(n_sto * sizeof(ZhBufDesc)), o_pieces = fa.reserve(n_piece * sizeof(ZhPieceDesc)),
                 o_er = fa.reserve(n_walk * 8);
    const size_t fa_in = fa.size;
    const size_t o_pcrc = fa.reserve(n_piece * 4), o_pad = fa.reserve(n_piece * 4), o_plen = fa.reserve(n_piece * 4),
                 o_scrc = fa.reserve(n_sto * 4), o_sad = fa.reserve(n_sto * 4), o_est = fa.reserve(n_slot * 4),
                 o_elen = fa.reserve(n_slot * 8), o_ebad = fa.reserve(n_walk * 4), o_eany = fa.reserve(n_walk * 4);
    if (dev_alloc(ctx, d_fin, fa.size + 256) != hipSuccess) return ZH_ERR_NOMEM;
    {
      std::vector<uint8_t> h(fa_in);
      memcpy(h.data() + o_fins, fins.data(), n_slot * sizeof(ZhZipFin));
      memcpy(h.data() + o_tasks, tasks.data(), n_task * sizeof(ZhZipFinTask));
      if (n_sto) memcpy(h.data() + o_sbufs, sbufs.data(), n_sto * sizeof(ZhBufDesc));
      if (n_piece) memcpy(h.data() + o_pieces, pieces.data(), n_piece * sizeof(ZhPieceDesc));
      memcpy(h.data() + o_er, eranges.data(), n_walk * 8);
      const void* src = h.data();
      if ((st = zhh_upload_slices(ctx, &src, {0}, {(uint64_t)fa_in}, fa_in, d_fin.p))) return st;
    }
    PlanGuard pg;
    if (n_def) {
      if ((st = zh_plan_uncompress(ctx, n_def, p_soff.data(), p_slen.data(), p_doff.data(), p_dcap.data(),
                                   ZH_DF_DEFLATE, &pg.p)) ||
          (st = zh_plan_request_crc32(pg.p, 1)))
        return st;
      if (tr.on) zh_plan_set_profiling(pg.p, 1);
      if ((st = zh_plan_run(pg.p, d_in.p, d_out.p))) return st;
      if (tr.on) {
        const char* names[64];
        float ms[64];
        const int nk = zh_plan_kernel_times(pg.p, names, ms, 64);
        for (int i = 0; i < nk && i < 64; i++) fprintf(stderr, "[zh]   plan kernel %-24s %8.3f ms\n", names[i], ms[i]);
      }
    }
    tr.mark(ctx, "zip open: decode");
    zh_launch_checksum_pieces(s, ctx->cktabs, d_in.p, carve<ZhPieceDesc>(d_fin.p, o_pieces), (uint32_t)n_piece, nullptr,
                              1, 0, carve<uint32_t>(d_fin.p, o_pcrc), carve<uint32_t>(d_fin.p, o_pad),
                              carve<uint32_t>(d_fin.p, o_plen));
    zh_launch_checksum_combine(s, ctx->cktabs, carve<ZhBufDesc>(d_fin.p, o_sbufs), (uint32_t)n_sto,
                               carve<uint32_t>(d_fin.p, o_pcrc), carve<uint32_t>(d_fin.p, o_pad),
                               carve<uint32_t>(d_fin.p, o_plen), 1, 0, carve<uint32_t>(d_fin.p, o_scrc),
                               carve<uint32_t>(d_fin.p, o_sad));
    // (plain pointers: a launch must not take the guard of the plan along)
    const int32_t* const plan_st = n_def ? zh_plan_device_statuses(pg.p) : nullptr;
    const uint64_t* const plan_len = n_def ? zh_plan_device_lens(pg.p) : nullptr;
    const uint32_t* const plan_crc = n_def ? pg.p->buf_crc : nullptr;
    const uint8_t* const in = d_in.p;
    uint8_t* const outp = d_out.p;
    hipLaunchKernelGGL(zh_zip_finish_kernel, dim3(((uint32_t)n_task + 3) / 4), wg, 0, s, in, outp,
                       (const ZhZipFin*)carve<ZhZipFin>(d_fin.p, o_fins),
                       (const ZhZipFinTask*)carve<ZhZipFinTask>(d_fin.p, o_tasks), (uint32_t)n_task,
                       plan_st, plan_len, plan_crc,
                       (const uint32_t*)carve<uint32_t>(d_fin.p, o_scrc), carve<int32_t>(d_fin.p, o_est),
                       carve<uint64_t>(d_fin.p, o_elen));
    hipLaunchKernelGGL(zh_zip_reduce_kernel, dim3((uint32_t)n_walk), wg, 0, s,
                       (const uint32_t*)carve<uint32_t>(d_fin.p, o_er), (const int32_t*)carve<int32_t>(d_fin.p, o_est),
                       (const uint8_t*)nullptr, carve<uint32_t>(d_fin.p, o_ebad), carve<uint32_t>(d_fin.p, o_eany));
    ZH_HIP(ctx, hipGetLastError());
    ZH_HIP(ctx, hipMemcpyAsync(est.data(), d_fin.p + o_est, n_slot * 4, hipMemcpyDeviceToHost, s));
    ZH_HIP(ctx, hipMemcpyAsync(elen.data(), d_fin.p + o_elen, n_slot * 8, hipMemcpyDeviceToHost, s));
    ZH_HIP(ctx, hipMemcpyAsync(ebad.data(), d_fin.p + o_ebad, n_walk * 4, hipMemcpyDeviceToHost, s));
    ZH_HIP(ctx, hipStreamSynchronize(s));
    tr.mark(ctx, "zip open: finish");

    // ---- 8. one download: every archive's block ----
    std::vector<char> take(n_walk, 0);
    for (size_t k = 0; k < n_walk; k++) take[k] = made.r[k] && ast[k] == ZH_OK && alen[k] ? 1 : 0;
    std::vector<size_t> blen(n_walk, 0);
    std::vector<int32_t> bst(n_walk, ZH_OK);
    st = zhh_download(ctx, d_out.p, n_walk, aoff, alen, take, blocks.data(), blen.data(), bst.data());
    blocks_at = own.p.size();
    own.p.insert(own.p.end(), blocks.begin(), blocks.end());
    if (st) return st;
    for (size_t k = 0; k < n_walk; k++)
      if (take[k] && bst[k]) return bst[k];  // (allocation)
    tr.mark(ctx, "zip open: download");
  }

  // An entry that outgrew its slot has a directory that understates its size; the reference does not look at the
  // size field, only at the CRC.  Such entries take zh_zip_extract_batch's own route, from the host image, all of
  // the call in one batch (rare: the CRC of these is compared here).
  std::vector<void*> redone(n_slot, nullptr);
  {
    std::vector<size_t> redo;
    for (size_t j = 0; j < n_slot; j++)
      if (est[j] == ZH_ERR_DST_TOO_SMALL) redo.push_back(j);
    if (!redo.empty()) {
      const size_t nr = redo.size();
      std::vector<const void*> rsrc(nr);
      std::vector<size_t> rlen(nr), rout(nr);
      std::vector<uint64_t> rhint(nr);
      std::vector<void*> rdst(nr, nullptr);
      std::vector<int32_t> rst(nr);
      std::vector<uint32_t> rcrc(nr);
      std::vector<char> stale(n_walk, 0);
      for (size_t q = 0; q < nr; q++) {
        const Slot& sl = slots[redo[q]];
        rsrc[q] = (const uint8_t*)images[walk[sl.walk]] + (sl.rec->src_off - imgs[sl.walk].up_off);
        rlen[q] = (size_t)sl.rec->src_len;
        rhint[q] = sl.rec->cap;
      }
      st = zh_uncompress_batch_sized(ctx, rsrc.data(), rlen.data(), nr, ZH_DF_DEFLATE, rhint.data(), rdst.data(),
                                     rout.data(), rst.data(), rcrc.data());
      own.p.insert(own.p.end(), rdst.begin(), rdst.end());
      const size_t base = own.p.size() - nr;
      if (st) return st;
      for (size_t q = 0; q < nr; q++) {
        const size_t j = redo[q];
        est[j] = rst[q] == ZH_OK && rcrc[q] != slots[j].rec->crc ? ZH_ERR_ZIP_CRC : rst[q];
        elen[j] = est[j] == ZH_OK ? rout[q] : 0;
        if (est[j] == ZH_OK) {
          redone[j] = rdst[q];
          own.p[base + q] = nullptr;  // the reader's from here on
        }
        stale[slots[j].walk] = 1;
      }
      for (size_t q = 0; q < nr; q++) {  // the first failing entry of these archives, once more
        const size_t k = slots[redo[q]].walk;
        if (!stale[k]) continue;
        stale[k] = 0;
        ebad[k] = kNone;
        for (size_t j = slot_lo[k]; j < slot_hi[k]; j++)
          if (est[j] != ZH_OK) {
            ebad[k] = (uint32_t)j;
            break;
          }
      }
      tr.mark(ctx, "zip open: redo");
    }
  }

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
        for (; j < n_slot && slots[j].walk == k; j++) {
          const size_t i = slots[j].entry;
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
