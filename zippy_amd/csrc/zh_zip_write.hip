// Writing zip archives, for many in-memory archives at once, in both of the reference's formats:
//  - zh_zip_write_batch: writeZipArchive (src/zippy/ziparchives_v1.nim:371-486), the 32-bit layout;
//  - zh_zip_create_batch: createZipArchive (src/zippy/ziparchives.nim:455-634), the zip64 layout.
// One host driver (zip_write_core) and one kernel body (zip_write_wave) serve both; a Layout a format carries what
// differs.  The host checks the archives and sends the non-empty contents back to back to the device (zhh_upload); one
// compress plan deflates them all and computes their CRC-32s; from the compressed lengths the host lays every archive
// out in one image buffer; the kernel then writes every byte of every image exactly once -- local headers and paths,
// the compressed streams gathered from the plan's output slots to their (unaligned) places, the central directory
// records, the end records -- through zh_gather.h's write_range; one download hands the images out.
#include <string_view>
#include <type_traits>
#include <unordered_set>

#include "zh_host.h"
#include "zh_gather.h"

namespace {

// One wave's work.  kTaskSlice / kTaskFirst: the image range [lo, hi) of entry idx's local part (a slice of at most
// kSlice stream bytes; the first slice with everything in front of the stream, and its wave also writes the entry's
// central directory record); kTaskEnd: archive idx's end records -- a task of their own, since a zip64 archive without
// entries has no other.
enum : uint32_t { kTaskSlice = 0, kTaskFirst = 1, kTaskEnd = 2 };
struct ZhZipTask {
  uint64_t lo, hi;
  uint32_t idx, kind;
};

constexpr uint64_t kSlice = 32768;  // stream bytes a wave copies at most
constexpr uint32_t kLocalSig = 0x04034b50u, kCentralSig = 0x02014b50u, kEocdSig = 0x06054b50u;
constexpr uint32_t kZip64EndSig = 0x06064b50u, kZip64LocatorSig = 0x07064b50u;
constexpr uint32_t kLocal64 = 30, kLocalExtra = 20, kCentral64 = 46, kCentralExtra = 28, kEnd64 = 56 + 20 + 22;

// byte j of the little-endian field x (of up to eight bytes) that starts at byte `at`
template <class T>
__device__ __forceinline__ uint32_t le(T x, uint32_t j, uint32_t at) {
  using U = std::conditional_t<(sizeof(T) > 4), uint64_t, uint32_t>;
  return (uint32_t)((U)x >> (8 * (j - at))) & 0xffu;
}

// ---------------------------------------------------------------------------------------------------------------
// The 32-bit layout (ziparchives_v1.nim): entries first to last; a local header, the path, the stream; a central
// directory record and the path; one end of central directory record.
// ---------------------------------------------------------------------------------------------------------------

// One entry, for the kernel (64 bytes).  Its local header, path and compressed stream are the image range
// [lh, lh + 30 + plen + clen); its central directory record is [cd, cd + 46 + plen).  src: the stream's offset in
// the plan's output buffer; path: the path's offset in the name pool; rel: lh - the archive's first byte.
struct ZhZipEntryDesc {
  uint64_t lh, cd, src, path;
  uint32_t clen, ulen, crc, rel;
  uint16_t plen, method, time, date;
  uint32_t ext, pad;
};

// One archive's end of central directory record: the image range [at, at + 22).
struct ZhZipEocdDesc {
  uint64_t at;
  uint32_t count, cd_size, cd_off, pad;
};

// The image byte at offset j of an entry's local part (:379-420): the 30-byte header, the path, the stream.
struct LocalGen {
  const ZhZipEntryDesc& d;
  const uint8_t* __restrict__ pool;
  const uint8_t* __restrict__ slots;
  __device__ uint32_t byte(uint64_t q) const {
    const uint64_t j64 = q - d.lh;
    if (j64 >= 30) {
      const uint64_t k = j64 - 30;
      return k < d.plen ? pool[d.path + k] : slots[d.src + (k - d.plen)];
    }
    const uint32_t j = (uint32_t)j64;
    if (j < 4) return le(kLocalSig, j, 0);
    if (j < 6) return le(20, j, 4);         // version needed to extract
    if (j < 8) return le(0x0800u, j, 6);    // flags: UTF-8
    if (j < 10) return le(d.method, j, 8);
    if (j < 12) return le(d.time, j, 10);
    if (j < 14) return le(d.date, j, 12);
    if (j < 18) return le(d.crc, j, 14);
    if (j < 22) return le(d.clen, j, 18);
    if (j < 26) return le(d.ulen, j, 22);
    if (j < 28) return le(d.plen, j, 26);
    return 0;                               // extra field length
  }
};

// The image byte at offset j of an entry's central directory record (:431-467).
struct CentralGen {
  const ZhZipEntryDesc& d;
  const uint8_t* __restrict__ pool;
  __device__ uint32_t byte(uint64_t q) const {
    const uint32_t j = (uint32_t)(q - d.cd);
    if (j >= 46) return pool[d.path + (j - 46)];
    if (j < 4) return le(kCentralSig, j, 0);
    if (j < 6) return le(63, j, 4);         // version made by
    if (j < 8) return le(20, j, 6);         // version needed to extract
    if (j < 10) return le(0x0800u, j, 8);
    if (j < 12) return le(d.method, j, 10);
    if (j < 14) return le(d.time, j, 12);
    if (j < 16) return le(d.date, j, 14);
    if (j < 20) return le(d.crc, j, 16);
    if (j < 24) return le(d.clen, j, 20);
    if (j < 28) return le(d.ulen, j, 24);
    if (j < 30) return le(d.plen, j, 28);
    if (j < 38) return 0;                   // extra, comment length, disk, internal attributes
    if (j < 42) return le(d.ext, j, 38);
    return le(d.rel, j, 42);
  }
};

// The image byte at offset j of an end of central directory record (:469-477).
struct EocdGen {
  const ZhZipEocdDesc& e;
  __device__ uint32_t byte(uint64_t q) const {
    const uint32_t j = (uint32_t)(q - e.at);
    if (j < 4) return le(kEocdSig, j, 0);
    if (j < 8) return 0;                    // disk numbers
    if (j < 10) return le(e.count, j, 8);
    if (j < 12) return le(e.count, j, 10);
    if (j < 16) return le(e.cd_size, j, 12);
    if (j < 20) return le(e.cd_off, j, 16);
    return 0;                               // comment length
  }
};

// ZH_ZIP32_LIMIT: the bound of the 32-bit fields checked after compression (default 2^32; read at each call, so that
// the tests can reach the refusal with small archives)
uint64_t zip32_limit() {
  const char* e = getenv("ZH_ZIP32_LIMIT");
  const long long v = e ? atoll(e) : 0;
  return v > 0 && (uint64_t)v < (1ull << 32) ? (uint64_t)v : 1ull << 32;
}

// splitFile(path).name is empty exactly when the path is empty or ends in '/' (std/os, POSIX)
bool stored_name(const zh_zip_new_entry& e) { return e.path_len == 0 || e.path[e.path_len - 1] == '/'; }

// steps 1-4 of the statuses (include/zippy_hip.h), before anything is read
int check_archive(const zh_zip_new_entry* es, size_t n) {
  if (!n) return ZH_ERR_ZIP_EMPTY;  // :375-376
  if (n > 0xffffu) return ZH_ERR_ZIP_TOO_LARGE;
  for (size_t i = 0; i < n; i++)
    if (es[i].path_len > 0xffffu || es[i].len >= (1ull << 32)) return ZH_ERR_ZIP_TOO_LARGE;
  for (size_t i = 0; i < n; i++)
    if (es[i].len && stored_name(es[i])) return ZH_ERR_ARGUMENT;
  std::unordered_set<std::string_view> seen;
  seen.reserve(n);
  for (size_t i = 0; i < n; i++)
    if (!seen.insert(std::string_view(es[i].path ? es[i].path : "", es[i].path_len)).second)
      return ZH_ERR_ZIP_DUPLICATE;
  return ZH_OK;
}

// What zip_write_core and zip_write_wave ask of a format.  kLocal / kCentral: the fixed bytes of an entry's local part
// and of its central directory record, beside the path (and the stream); kEnd: the end records.  limit(): what an
// entry's compressed length, a local header's offset and the central directory's size and offset stay below (step 5).
struct Zip32Layout {
  using Entry = ZhZipEntryDesc;
  using End = ZhZipEocdDesc;
  using Local = LocalGen;
  using Central = CentralGen;
  using EndRecords = EocdGen;
  static constexpr const char* kTrace = "zip";
  static constexpr bool kLastToFirst = false;
  static constexpr uint32_t kLocal = 30, kCentral = 46, kEnd = 22;
  static int check(const zh_zip_new_entry* es, size_t n) { return check_archive(es, n); }
  static uint64_t limit() { return zip32_limit(); }
  // (method 0 with contents was refused in step 3)
  static Entry entry(const zh_zip_new_entry& e, uint64_t lh, uint64_t cd, uint64_t src, uint64_t path, uint64_t clen,
                     uint32_t crc, uint64_t rel, uint16_t method) {
    return {lh, cd, src, path, (uint32_t)clen, (uint32_t)e.len, crc, (uint32_t)rel, (uint16_t)e.path_len, method,
            e.dos_time, e.dos_date, e.is_directory ? 0x10u : 0x20u, 0};
  }
  static End end(uint64_t at, uint64_t count, uint64_t cd_size, uint64_t cd_off) {
    return {at, (uint32_t)count, (uint32_t)cd_size, (uint32_t)cd_off, 0};
  }
};

// ---------------------------------------------------------------------------------------------------------------
// The zip64 layout (ziparchives.nim).  Entries are laid out last to first (the reference pops keys off the table's
// end, :503-505); every local header is followed by its path, a 20-byte zip64 extra and the stream; every central
// directory record by its path and a 28-byte extra; three end records (98 bytes) close the archive.  All lengths and
// offsets are 64-bit, in the descriptors and in the image.
// ---------------------------------------------------------------------------------------------------------------

// One entry, for the kernel.  Its local part is the image range [lh, lh + 30 + plen + 20 + clen), its central
// directory record [cd, cd + 46 + plen + 28).  src / path / rel: as in ZhZipEntryDesc.
struct ZhZip64EntryDesc {
  uint64_t lh, cd, src, path, clen, ulen, rel;
  uint32_t crc;
  uint16_t plen, method, time, date;
};

// One archive's end records: the image range [at, at + 98).  cd_off: the central directory's offset in the archive.
struct ZhZip64EndDesc {
  uint64_t at, count, cd_size, cd_off;
};

// The image byte at offset j of an entry's local part (:541-566): the header, the path, the zip64 extra, the stream.
struct Local64Gen {
  const ZhZip64EntryDesc& d;
  const uint8_t* __restrict__ pool;
  const uint8_t* __restrict__ slots;
  __device__ uint32_t byte(uint64_t q) const {
    const uint64_t j64 = q - d.lh;
    if (j64 >= kLocal64) {
      const uint64_t k = j64 - kLocal64;
      if (k < d.plen) return pool[d.path + k];
      const uint64_t x = k - d.plen;
      if (x >= kLocalExtra) return slots[d.src + (x - kLocalExtra)];
      const uint32_t j = (uint32_t)x;
      if (j < 2) return le(1, j, 0);          // zip64 extended information
      if (j < 4) return le(16, j, 2);
      if (j < 12) return le(d.ulen, j, 4);
      return le(d.clen, j, 12);
    }
    const uint32_t j = (uint32_t)j64;
    if (j < 4) return le(kLocalSig, j, 0);
    if (j < 6) return le(45, j, 4);           // version needed to extract
    if (j < 8) return le(0x0800u, j, 6);      // flags: UTF-8
    if (j < 10) return le(d.method, j, 8);
    if (j < 12) return le(d.time, j, 10);
    if (j < 14) return le(d.date, j, 12);
    if (j < 18) return le(d.crc, j, 14);
    if (j < 26) return 0xffu;                 // both lengths: in the extra
    if (j < 28) return le(d.plen, j, 26);
    return le(kLocalExtra, j, 28);
  }
};

// The image byte at offset j of an entry's central directory record (:570-596).
struct Central64Gen {
  const ZhZip64EntryDesc& d;
  const uint8_t* __restrict__ pool;
  __device__ uint32_t byte(uint64_t q) const {
    const uint32_t j = (uint32_t)(q - d.cd);
    if (j >= kCentral64) {
      const uint32_t k = j - kCentral64;
      if (k < d.plen) return pool[d.path + k];
      const uint32_t x = k - d.plen;
      if (x < 2) return le(1, x, 0);
      if (x < 4) return le(24, x, 2);
      if (x < 12) return le(d.ulen, x, 4);
      if (x < 20) return le(d.clen, x, 12);
      return le(d.rel, x, 20);
    }
    if (j < 4) return le(kCentralSig, j, 0);
    if (j < 6) return le(45, j, 4);           // version made by
    if (j < 8) return le(45, j, 6);           // version needed to extract
    if (j < 10) return le(0x0800u, j, 8);
    if (j < 12) return le(d.method, j, 10);
    if (j < 14) return le(d.time, j, 12);
    if (j < 16) return le(d.date, j, 14);
    if (j < 20) return le(d.crc, j, 16);
    if (j < 28) return 0xffu;                 // both lengths: in the extra
    if (j < 30) return le(d.plen, j, 28);
    if (j < 32) return le(kCentralExtra, j, 30);
    if (j < 42) return 0;                     // comment length, disk, internal and external attributes
    return 0xffu;                             // the local header's offset: in the extra
  }
};

// The image byte at offset j of an archive's end records (:600-623): the zip64 end of central directory record, its
// locator, the end of central directory record.
struct End64Gen {
  const ZhZip64EndDesc& e;
  __device__ __forceinline__ uint32_t byte(uint64_t q) const {  // (called twice a lane: a call would put e in scratch)
    const uint32_t j = (uint32_t)(q - e.at);
    if (j < 4) return le(kZip64EndSig, j, 0);
    if (j < 12) return le(44ull, j, 4);       // size of the rest of this record
    if (j < 14) return le(45, j, 12);
    if (j < 16) return le(45, j, 14);
    if (j < 24) return 0;                     // disk numbers
    if (j < 32) return le(e.count, j, 24);
    if (j < 40) return le(e.count, j, 32);
    if (j < 48) return le(e.cd_size, j, 40);
    if (j < 56) return le(e.cd_off, j, 48);
    if (j < 60) return le(kZip64LocatorSig, j, 56);
    if (j < 64) return 0;
    if (j < 72) return le(e.cd_off + e.cd_size, j, 64);  // where the zip64 end record starts
    if (j < 76) return le(1, j, 72);          // disks
    if (j < 80) return le(kEocdSig, j, 76);
    if (j < 84) return 0;
    if (j < 96) return 0xffu;                 // counts, size, offset: in the zip64 record
    return 0;                                 // comment length
  }
};

// the statuses of include/zippy_hip.h: entry by entry in processing order (last to first, :503-511)
int check_archive64(const zh_zip_new_entry* es, size_t n) {
  std::unordered_set<std::string_view> seen;
  seen.reserve(n);
  for (size_t i = n; i-- > 0;) {
    if (es[i].path_len == 0) return ZH_ERR_ZIP_NAME;       // "Invalid empty file name"
    if (es[i].path[0] == '/') return ZH_ERR_ZIP_NAME;      // "File paths must be relative"
    if (es[i].path_len > 0xffffu) return ZH_ERR_ZIP_NAME;  // "File name len > uint16.high"
    if (!seen.insert(std::string_view(es[i].path, es[i].path_len)).second) return ZH_ERR_ZIP_DUPLICATE;
  }
  return ZH_OK;
}

struct Zip64Layout {
  using Entry = ZhZip64EntryDesc;
  using End = ZhZip64EndDesc;
  using Local = Local64Gen;
  using Central = Central64Gen;
  using EndRecords = End64Gen;
  static constexpr const char* kTrace = "zip64";
  static constexpr bool kLastToFirst = true;
  static constexpr uint32_t kLocal = kLocal64 + kLocalExtra, kCentral = kCentral64 + kCentralExtra, kEnd = kEnd64;
  static int check(const zh_zip_new_entry* es, size_t n) { return check_archive64(es, n); }
  static uint64_t limit() { return ~0ull; }  // every field is 64-bit: nothing to refuse
  static Entry entry(const zh_zip_new_entry& e, uint64_t lh, uint64_t cd, uint64_t src, uint64_t path, uint64_t clen,
                     uint32_t crc, uint64_t rel, uint16_t method) {
    return {lh, cd, src, path, clen, e.len, rel, crc, (uint16_t)e.path_len, method, e.dos_time, e.dos_date};
  }
  static End end(uint64_t at, uint64_t count, uint64_t cd_size, uint64_t cd_off) {
    return {at, count, cd_size, cd_off};
  }
};

// One wave per task (four a workgroup): a slice of an entry's local part (the first slice's wave also writes the
// entry's central directory record), or an archive's end records.  The task is the wave's, so the branches are uniform.
template <class L>
__device__ __forceinline__ void zip_write_wave(uint8_t* __restrict__ img, const uint8_t* __restrict__ slots,
                                               const typename L::Entry* __restrict__ descs,
                                               const ZhZipTask* __restrict__ tasks, uint64_t n_tasks,
                                               const typename L::End* __restrict__ ends,
                                               const uint8_t* __restrict__ pool) {
  const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (wave >= n_tasks) return;
  const ZhZipTask t = tasks[wave];
  if (t.kind != kTaskEnd) {
    const typename L::Entry d = descs[t.idx];
    write_range(img, t.lo, t.hi, lane, typename L::Local{d, pool, slots}, d.lh + L::kLocal + d.plen, slots, d.src);
    if (t.kind == kTaskFirst) write_range(img, d.cd, d.cd + L::kCentral + d.plen, lane, typename L::Central{d, pool});
  } else {
    const typename L::End e = ends[t.idx];
    // 22 or 98 bytes, [t.lo, t.hi): a byte a lane a round.  (Through write_range, the sixteen field ladders of a chunk
    // of these records set the register need of the whole kernel: 96 to 136 VGPRs against 62 for the entries' part.)
    const typename L::EndRecords g{e};
#pragma unroll
    for (uint32_t j0 = 0; j0 < L::kEnd; j0 += 64)
      if (j0 + lane < L::kEnd) img[t.lo + j0 + lane] = (uint8_t)g.byte(t.lo + j0 + lane);
  }
}

}  // namespace

__global__ __launch_bounds__(256) void zh_zip_write_kernel(uint8_t* __restrict__ img, const uint8_t* __restrict__ slots,
                                                           const ZhZipEntryDesc* __restrict__ descs,
                                                           const ZhZipTask* __restrict__ tasks, uint64_t n_tasks,
                                                           const ZhZipEocdDesc* __restrict__ eocds,
                                                           const uint8_t* __restrict__ pool) {
  zip_write_wave<Zip32Layout>(img, slots, descs, tasks, n_tasks, eocds, pool);
}

__global__ __launch_bounds__(256) void zh_zip_create_kernel(uint8_t* __restrict__ img, const uint8_t* __restrict__ slots,
                                                            const ZhZip64EntryDesc* __restrict__ descs,
                                                            const ZhZipTask* __restrict__ tasks, uint64_t n_tasks,
                                                            const ZhZip64EndDesc* __restrict__ ends,
                                                            const uint8_t* __restrict__ pool) {
  zip_write_wave<Zip64Layout>(img, slots, descs, tasks, n_tasks, ends, pool);
}

namespace {

uint64_t round_up(uint64_t x, uint64_t a) { return (x + a - 1) & ~(a - 1); }

// Both batch calls behind their argument checks: L's archives from the tables, written by `kernel` (the __global__
// name of zip_write_wave<L>).
template <class L, class Kernel>
int zip_write_core(Kernel kernel, zh_ctx* ctx, const zh_zip_new_entry* entries, const size_t* first, size_t n_zip,
                   int level, void** dsts, size_t* dst_lens, int32_t* statuses) {
  const std::string mark = std::string(L::kTrace) + ": ";
  // entry number j of archive [i0, i1) in processing order
  auto nth = [](size_t i0, size_t i1, size_t j) { return L::kLastToFirst ? i1 - 1 - j : i0 + j; };

  // ---- the checks; the non-empty contents of the archives that pass, in processing order, in one device buffer ----
  std::vector<size_t> ok;  // the archives still in the running, in order
  std::vector<const void*> csrc;
  std::vector<size_t> clens;
  std::vector<uint32_t> slot_of(first[n_zip] - first[0], ~0u);  // entry -> its plan buffer
  for (size_t t = 0; t < n_zip; t++) {
    const size_t i0 = first[t], i1 = first[t + 1];
    if ((statuses[t] = L::check(entries + i0, i1 - i0)) != ZH_OK) continue;
    ok.push_back(t);
    for (size_t j = 0; j < i1 - i0; j++) {
      const size_t i = nth(i0, i1, j);
      if (!entries[i].len) continue;
      slot_of[i - first[0]] = (uint32_t)csrc.size();
      csrc.push_back(entries[i].contents);
      clens.push_back(entries[i].len);
    }
  }
  if (ok.empty()) return ZH_OK;
  ZH_HIP(ctx, hipSetDevice(ctx->device));
  Trace tr;
  DevBuf d_src, d_slots;
  std::vector<uint64_t> soff, slen;
  int st = ZH_OK;
  if (!csrc.empty() && (st = zhh_upload(ctx, csrc.data(), clens.data(), csrc.size(), d_src, soff, slen))) return st;
  tr.mark(ctx, (mark + "upload").c_str());

  // ---- compress(contents, level, dfDeflate) and crc32(contents) of every non-empty entry: one plan ----
  std::vector<uint64_t> doff, clen;
  std::vector<int32_t> cst;
  std::vector<uint32_t> crc(csrc.size(), 0);
  if ((st = zhh_compress(ctx, d_src.p, soff, slen, level, ZH_DF_DEFLATE, crc.data(), d_slots, doff, clen, cst)))
    return st;
  tr.mark(ctx, (mark + "compress").c_str());
  if (d_src.p) {  // (back to the context's cache before the image is allocated)
    ctx_free(ctx, d_src.p);
    d_src.p = nullptr;
  }

  // ---- what compression decides (step 5) and the layout: archive t's image is [img_off, + img_len) of one buffer,
  // 256-aligned ----
  const uint64_t lim = L::limit();
  std::vector<typename L::Entry> descs;
  std::vector<ZhZipTask> tasks;
  std::vector<typename L::End> ends;
  std::vector<uint8_t> pool;
  std::vector<size_t> done;  // the archives that are written, in order
  std::vector<uint64_t> img_off, img_len;
  uint64_t o = 0;
  for (size_t t : ok) {
    const size_t i0 = first[t], i1 = first[t + 1];
    int ast = ZH_OK;
    uint64_t at = 0, names = 0;  // (offsets inside the archive)
    for (size_t j = 0; j < i1 - i0 && ast == ZH_OK; j++) {
      const size_t i = nth(i0, i1, j);
      const uint32_t k = slot_of[i - first[0]];
      const uint64_t c = k == ~0u ? 0 : clen[k];
      if (k != ~0u && cst[k] != ZH_OK) ast = cst[k];
      else if (at >= lim || c >= lim) ast = ZH_ERR_ZIP_TOO_LARGE;
      at += L::kLocal + entries[i].path_len + c;
      names += entries[i].path_len;
    }
    const uint64_t cd_size = (uint64_t)L::kCentral * (i1 - i0) + names;
    if (ast == ZH_OK && (at >= lim || cd_size >= lim)) ast = ZH_ERR_ZIP_TOO_LARGE;
    if (ast != ZH_OK) {
      statuses[t] = ast;
      continue;
    }
    done.push_back(t);
    img_off.push_back(o);
    uint64_t cd = o + at;
    for (size_t j = 0; j < i1 - i0; j++) {
      const size_t i = nth(i0, i1, j);
      const zh_zip_new_entry& e = entries[i];
      const uint32_t k = slot_of[i - first[0]];
      const uint64_t c = k == ~0u ? 0 : clen[k];
      const uint32_t idx = (uint32_t)descs.size();
      descs.push_back(L::entry(e, o, cd, k == ~0u ? 0 : doff[k], pool.size(), c, k == ~0u ? 0 : crc[k],
                               o - img_off.back(), k == ~0u ? 0 : 8));
      if (e.path_len) pool.insert(pool.end(), (const uint8_t*)e.path, (const uint8_t*)e.path + e.path_len);
      const uint64_t data_at = o + L::kLocal + e.path_len, end = data_at + c;
      uint64_t lo = o;
      for (uint64_t hi = std::min(end, data_at + kSlice);; hi = std::min(end, hi + kSlice)) {
        tasks.push_back({lo, hi, idx, lo == o ? kTaskFirst : kTaskSlice});
        if ((lo = hi) == end) break;
      }
      o = end;
      cd += L::kCentral + e.path_len;
    }
    tasks.push_back({cd, cd + L::kEnd, (uint32_t)ends.size(), kTaskEnd});
    ends.push_back(L::end(cd, i1 - i0, cd_size, at));
    img_len.push_back(cd + L::kEnd - img_off.back());
    o = round_up(cd + L::kEnd, 256);
  }
  const size_t n_done = done.size();
  if (!n_done) return ZH_OK;

  // ---- descriptors, tasks, end records and names in one upload ----
  DevBuf d_meta, d_img;
  std::vector<uint64_t> moff;
  if ((st = zhh_upload_spans(ctx, {{descs.data(), descs.size() * sizeof(typename L::Entry)},
                                   {tasks.data(), tasks.size() * sizeof(ZhZipTask)},
                                   {ends.data(), ends.size() * sizeof(typename L::End)}, {pool.data(), pool.size()}},
                             d_meta, moff)))
    return st;
  if (dev_alloc(ctx, d_img, o + 256) != hipSuccess) return ZH_ERR_NOMEM;
  tr.mark(ctx, (mark + "layout").c_str());

  uint8_t* const img = d_img.p;  // (plain pointers into the launch: a DevBuf is not to be copied)
  const uint8_t *const mp = d_meta.p, *const slots = d_slots.p;
  constexpr uint64_t kGridTasks = 4ull << 22;  // tasks a launch: 2^22 workgroups
  for (uint64_t t0 = 0; t0 < tasks.size(); t0 += kGridTasks) {
    const uint64_t nt = std::min<uint64_t>(kGridTasks, tasks.size() - t0);
    hipLaunchKernelGGL(kernel, dim3((uint32_t)((nt + 3) / 4)), dim3(256), 0, ctx->stream, img, slots,
                       reinterpret_cast<const typename L::Entry*>(mp + moff[0]),
                       reinterpret_cast<const ZhZipTask*>(mp + moff[1]) + t0, nt,
                       reinterpret_cast<const typename L::End*>(mp + moff[2]), mp + moff[3]);
    ZH_HIP(ctx, hipGetLastError());
  }
  tr.mark(ctx, (mark + "write").c_str());

  if ((st = writer_hand_out(ctx, d_img.p, done, img_off, img_len, std::vector<int32_t>(n_done, ZH_OK), dsts,
                            dst_lens, statuses)))
    return st;
  tr.mark(ctx, (mark + "download").c_str());
  return ZH_OK;
}

}  // namespace

extern "C" int zh_zip_write_batch(zh_ctx* ctx, const zh_zip_new_entry* entries, const size_t* first, size_t n_zip,
                                  int level, void** dsts, size_t* dst_lens, int32_t* statuses) {
  if (const int st = writer_checks(ctx, entries, first, n_zip, level < -2 || level > 9 ? ZH_ERR_INVALID_LEVEL : ZH_OK,
                                   dsts, dst_lens, statuses);
      st || !n_zip)
    return st;
  return zip_write_core<Zip32Layout>(zh_zip_write_kernel, ctx, entries, first, n_zip, level, dsts, dst_lens, statuses);
}

extern "C" int zh_zip_create_batch(zh_ctx* ctx, const zh_zip_new_entry* entries, const size_t* first, size_t n_zip,
                                   int level, void** dsts, size_t* dst_lens, int32_t* statuses) {
  if (const int st = writer_checks(ctx, entries, first, n_zip, level < -2 || level > 9 ? ZH_ERR_INVALID_LEVEL : ZH_OK,
                                   dsts, dst_lens, statuses);
      st || !n_zip)
    return st;
  // the tasks name entries and archives in 32 bits (tasks themselves are counted in 64)
  if (first[n_zip] - first[0] >= 0xffffffffull || n_zip >= 0xffffffffull) return ZH_ERR_ARGUMENT;
  return zip_write_core<Zip64Layout>(zh_zip_create_kernel, ctx, entries, first, n_zip, level, dsts, dst_lens, statuses);
}
