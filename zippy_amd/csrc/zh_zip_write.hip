// Writing zip archives: writeZipArchive (src/zippy/ziparchives_v1.nim:371-486) for many in-memory archives at once.
// The host checks the archives and sends the non-empty contents back to back to the device (zhh_upload_slices); one
// compress plan deflates them all and computes their CRC-32s; from the compressed lengths the host lays every
// archive out in one image buffer; zh_zip_write_kernel then writes every byte of every image exactly once -- local
// headers and paths, the compressed streams gathered from the plan's output slots to their (unaligned) places, the
// central directory records, the end of central directory records --; one download hands the images out.
// Further down: createZipArchive (src/zippy/ziparchives.nim:455-634) the same way, zh_zip_create_batch and
// zh_zip_create_kernel, with the zip64 layout; the two kernels share write_range / gather16 / bytes16.
#include <string_view>
#include <unordered_set>

#include "zh_host.h"
#include "zh_gather.h"

namespace {

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

// One wave's work: the image range [lo, hi) of entry `entry`'s local part (a slice of at most kSlice stream bytes,
// the first slice with the header and the path).  The first slice of an entry also writes its central directory
// record; eocd != 0: this wave also writes archive eocd - 1's end record.
struct ZhZipTask {
  uint64_t lo, hi;
  uint32_t entry, first, eocd, pad;
};

constexpr uint64_t kSlice = 32768;  // stream bytes a wave copies at most
constexpr uint32_t kLocalSig = 0x04034b50u, kCentralSig = 0x02014b50u, kEocdSig = 0x06054b50u;

// byte j of the little-endian field x that starts at byte `at`
__device__ __forceinline__ uint32_t le(uint32_t x, uint32_t j, uint32_t at) { return (x >> (8 * (j - at))) & 0xffu; }

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

template <class Gen>
__device__ __forceinline__ Chunk16 bytes16(const Gen& g, uint64_t c) {
  Chunk16 v{{0, 0, 0, 0}};
#pragma unroll
  for (uint32_t k = 0; k < 16; k++) v.w[k >> 2] |= g.byte(c + k) << (8 * (k & 3));
  return v;
}

// One wave writes the image range [a, b): the bytes in front of the first and behind the last aligned 16-byte chunk
// one a lane, every whole chunk in between with one 16-byte store.  Ranges of different waves never share a byte,
// so no byte of an image is written twice.  Chunks at or past `copy_at` take their bytes straight from
// slots + copy_src + (chunk - copy_at).
template <class Gen>
__device__ __forceinline__ void write_range(uint8_t* __restrict__ img, uint64_t a, uint64_t b, uint32_t lane,
                                            const Gen& g, uint64_t copy_at = ~0ull,
                                            const uint8_t* __restrict__ slots = nullptr, uint64_t copy_src = 0) {
  if (a >= b) return;
  const uint64_t A = (a + 15) & ~(uint64_t)15, B = b & ~(uint64_t)15;
  if (A >= B) {  // no whole chunk inside: at most 30 bytes
    if (a + lane < b) img[a + lane] = (uint8_t)g.byte(a + lane);
    return;
  }
  if (a + lane < A) img[a + lane] = (uint8_t)g.byte(a + lane);
  if (B + lane < b) img[B + lane] = (uint8_t)g.byte(B + lane);
  for (uint64_t c = A + 16ull * lane; c < B; c += 1024) {
    const Chunk16 v = c >= copy_at ? gather16(slots, copy_src + (c - copy_at)) : bytes16(g, c);
    *reinterpret_cast<Chunk16*>(img + c) = v;
  }
}

}  // namespace

// One wave per task (four a workgroup): a slice of an entry's local part; the first slice's wave also writes the
// entry's central directory record, the wave of an archive's last entry also its end record.
__global__ __launch_bounds__(256) void zh_zip_write_kernel(uint8_t* __restrict__ img, const uint8_t* __restrict__ slots,
                                                           const ZhZipEntryDesc* __restrict__ descs,
                                                           const ZhZipTask* __restrict__ tasks, uint64_t n_tasks,
                                                           const ZhZipEocdDesc* __restrict__ eocds,
                                                           const uint8_t* __restrict__ pool) {
  const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (wave >= n_tasks) return;
  const ZhZipTask t = tasks[wave];
  const ZhZipEntryDesc d = descs[t.entry];
  const uint64_t data_at = d.lh + 30 + d.plen;
  write_range(img, t.lo, t.hi, lane, LocalGen{d, pool, slots}, data_at, slots, d.src);
  if (t.first) write_range(img, d.cd, d.cd + 46 + d.plen, lane, CentralGen{d, pool});
  if (t.eocd) {
    const ZhZipEocdDesc e = eocds[t.eocd - 1];
    write_range(img, e.at, e.at + 22, lane, EocdGen{e});
  }
}

namespace {

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

uint64_t round_up(uint64_t x, uint64_t a) { return (x + a - 1) & ~(a - 1); }

}  // namespace

extern "C" int zh_zip_write_batch(zh_ctx* ctx, const zh_zip_new_entry* entries, const size_t* first, size_t n_zip,
                                  int level, void** dsts, size_t* dst_lens, int32_t* statuses) {
  if (const int st = writer_checks(ctx, entries, first, n_zip, level < -2 || level > 9 ? ZH_ERR_INVALID_LEVEL : ZH_OK,
                                   dsts, dst_lens, statuses);
      st || !n_zip)
    return st;

  // ---- steps 1-4; the non-empty contents of the archives that pass, 256-aligned in one device buffer ----
  std::vector<size_t> ok;                    // the archives still in the running, in order
  std::vector<const void*> csrc;
  std::vector<size_t> clens;
  std::vector<uint32_t> slot_of(first[n_zip] - first[0], ~0u);  // entry -> its plan buffer
  for (size_t t = 0; t < n_zip; t++) {
    if ((statuses[t] = check_archive(entries + first[t], first[t + 1] - first[t])) != ZH_OK) continue;
    ok.push_back(t);
    for (size_t i = first[t]; i < first[t + 1]; i++) {
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
  tr.mark(ctx, "zip: upload");

  // ---- compress(contents, level, dfDeflate) and crc32(contents) of every non-empty entry: one plan ----
  std::vector<uint64_t> doff, clen;
  std::vector<int32_t> cst;
  std::vector<uint32_t> crc(csrc.size(), 0);
  if ((st = zhh_compress(ctx, d_src.p, soff, slen, level, ZH_DF_DEFLATE, crc.data(), d_slots, doff, clen, cst)))
    return st;
  tr.mark(ctx, "zip: compress");
  if (d_src.p) {  // (back to the context's cache before the image is allocated)
    ctx_free(ctx, d_src.p);
    d_src.p = nullptr;
  }

  // ---- step 5 and the layout: archive t's image is [img_off, + img_len) of one buffer, 256-aligned ----
  const uint64_t lim = zip32_limit();
  std::vector<ZhZipEntryDesc> descs;
  std::vector<ZhZipTask> tasks;
  std::vector<ZhZipEocdDesc> eocds;
  std::vector<uint8_t> pool;
  std::vector<size_t> done;  // the archives that are written, in order
  std::vector<uint64_t> img_off, img_len;
  uint64_t o = 0;
  for (size_t t : ok) {
    const size_t i0 = first[t], i1 = first[t + 1];
    int ast = ZH_OK;
    uint64_t at = 0, names = 0;  // (offsets inside the archive)
    for (size_t i = i0; i < i1 && ast == ZH_OK; i++) {
      const uint32_t k = slot_of[i - first[0]];
      const uint64_t c = k == ~0u ? 0 : clen[k];
      if (k != ~0u && cst[k] != ZH_OK) ast = cst[k];
      else if (at >= lim || c >= lim) ast = ZH_ERR_ZIP_TOO_LARGE;
      at += 30 + entries[i].path_len + c;
      names += entries[i].path_len;
    }
    const uint64_t cd_size = 46 * (i1 - i0) + names;
    if (ast == ZH_OK && (at >= lim || cd_size >= lim)) ast = ZH_ERR_ZIP_TOO_LARGE;
    if (ast != ZH_OK) {
      statuses[t] = ast;
      continue;
    }
    done.push_back(t);
    img_off.push_back(o);
    uint64_t cd = o + at;
    for (size_t i = i0; i < i1; i++) {
      const zh_zip_new_entry& e = entries[i];
      const uint32_t k = slot_of[i - first[0]];
      ZhZipEntryDesc d{};
      d.lh = o;
      d.cd = cd;
      d.src = k == ~0u ? 0 : doff[k];
      d.path = pool.size();
      d.clen = k == ~0u ? 0 : (uint32_t)clen[k];
      d.ulen = (uint32_t)e.len;
      d.crc = k == ~0u ? 0 : crc[k];
      d.rel = (uint32_t)(o - img_off.back());
      d.plen = (uint16_t)e.path_len;
      d.method = k == ~0u ? 0 : 8;  // (method 0 with contents was refused in step 3)
      d.time = e.dos_time;
      d.date = e.dos_date;
      d.ext = e.is_directory ? 0x10u : 0x20u;
      if (e.path_len) pool.insert(pool.end(), (const uint8_t*)e.path, (const uint8_t*)e.path + e.path_len);
      const uint32_t idx = (uint32_t)descs.size();
      descs.push_back(d);
      const uint64_t end = o + 30 + e.path_len + d.clen;
      uint64_t lo = o;
      for (uint64_t hi = std::min(end, o + 30 + e.path_len + kSlice);; hi = std::min(end, hi + kSlice)) {
        tasks.push_back({lo, hi, idx, lo == o ? 1u : 0u, 0, 0});
        if ((lo = hi) == end) break;
      }
      o = end;
      cd += 46 + e.path_len;
    }
    eocds.push_back({cd, (uint32_t)(i1 - i0), (uint32_t)cd_size, (uint32_t)at, 0});
    // the end record goes with the archive's last entry's first slice
    for (size_t j = tasks.size(); j-- > 0;)
      if (tasks[j].first) {
        tasks[j].eocd = (uint32_t)eocds.size();
        break;
      }
    img_len.push_back(cd + 22 - img_off.back());
    o = round_up(cd + 22, 256);
  }
  const size_t n_done = done.size();
  if (!n_done) return ZH_OK;

  // ---- descriptors, tasks, end records and names in one upload ----
  DevBuf d_meta, d_img;
  std::vector<uint64_t> moff;
  if ((st = zhh_upload_spans(ctx, {{descs.data(), descs.size() * sizeof(ZhZipEntryDesc)},
                                   {tasks.data(), tasks.size() * sizeof(ZhZipTask)},
                                   {eocds.data(), eocds.size() * sizeof(ZhZipEocdDesc)}, {pool.data(), pool.size()}},
                             d_meta, moff)))
    return st;
  if (dev_alloc(ctx, d_img, o + 256) != hipSuccess) return ZH_ERR_NOMEM;
  tr.mark(ctx, "zip: layout");

  uint8_t* const img = d_img.p;  // (plain pointers into the launch: a DevBuf is not to be copied)
  const uint8_t *const mp = d_meta.p, *const slots = d_slots.p;
  constexpr uint64_t kGridTasks = 4ull << 22;  // tasks a launch: 2^22 workgroups
  for (uint64_t t0 = 0; t0 < tasks.size(); t0 += kGridTasks) {
    const uint64_t nt = std::min<uint64_t>(kGridTasks, tasks.size() - t0);
    hipLaunchKernelGGL(zh_zip_write_kernel, dim3((uint32_t)((nt + 3) / 4)), dim3(256), 0, ctx->stream, img,
                       slots, reinterpret_cast<const ZhZipEntryDesc*>(mp + moff[0]),
                       reinterpret_cast<const ZhZipTask*>(mp + moff[1]) + t0, nt,
                       reinterpret_cast<const ZhZipEocdDesc*>(mp + moff[2]), mp + moff[3]);
    ZH_HIP(ctx, hipGetLastError());
  }
  tr.mark(ctx, "zip: write");

  if ((st = writer_hand_out(ctx, d_img.p, done, img_off, img_len, std::vector<int32_t>(n_done, ZH_OK), dsts,
                            dst_lens, statuses)))
    return st;
  tr.mark(ctx, "zip: download");
  return ZH_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// createZipArchive(entries: OrderedTable[string, string]) (src/zippy/ziparchives.nim:455-634) for many in-memory
// archives at once: the same pipeline with the zip64 layout.  Entries are laid out last to first (the reference pops
// keys off the table's end, :503-505); every local header is followed by its path, a 20-byte zip64 extra and the
// stream; every central directory record by its path and a 28-byte extra; three end records (98 bytes) close the
// archive.  All lengths and offsets are 64-bit, in the descriptors and in the image.
// ---------------------------------------------------------------------------------------------------------------
namespace {

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

// One wave's work.  kTaskSlice / kTaskFirst: the image range [lo, hi) of entry idx's local part (the first slice with
// the header, the path and the extra; its wave also writes the entry's central directory record); kTaskEnd: archive
// idx's end records -- a task of their own, since an archive without entries has no other.
enum : uint32_t { kTaskSlice = 0, kTaskFirst = 1, kTaskEnd = 2 };
struct ZhZip64Task {
  uint64_t lo, hi;
  uint32_t idx, kind;
};

constexpr uint32_t kZip64EndSig = 0x06064b50u, kZip64LocatorSig = 0x07064b50u;
constexpr uint32_t kLocal64 = 30, kLocalExtra = 20, kCentral64 = 46, kCentralExtra = 28, kEnd64 = 56 + 20 + 22;

__device__ __forceinline__ uint32_t le64(uint64_t x, uint32_t j, uint32_t at) {
  return (uint32_t)(x >> (8 * (j - at))) & 0xffu;
}

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
      if (j < 12) return le64(d.ulen, j, 4);
      return le64(d.clen, j, 12);
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
      if (x < 12) return le64(d.ulen, x, 4);
      if (x < 20) return le64(d.clen, x, 12);
      return le64(d.rel, x, 20);
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
  __device__ uint32_t byte(uint64_t q) const {
    const uint32_t j = (uint32_t)(q - e.at);
    if (j < 4) return le(kZip64EndSig, j, 0);
    if (j < 12) return le64(44, j, 4);        // size of the rest of this record
    if (j < 14) return le(45, j, 12);
    if (j < 16) return le(45, j, 14);
    if (j < 24) return 0;                     // disk numbers
    if (j < 32) return le64(e.count, j, 24);
    if (j < 40) return le64(e.count, j, 32);
    if (j < 48) return le64(e.cd_size, j, 40);
    if (j < 56) return le64(e.cd_off, j, 48);
    if (j < 60) return le(kZip64LocatorSig, j, 56);
    if (j < 64) return 0;
    if (j < 72) return le64(e.cd_off + e.cd_size, j, 64);  // where the zip64 end record starts
    if (j < 76) return le(1, j, 72);          // disks
    if (j < 80) return le(kEocdSig, j, 76);
    if (j < 84) return 0;
    if (j < 96) return 0xffu;                 // counts, size, offset: in the zip64 record
    return 0;                                 // comment length
  }
};

}  // namespace

// One wave per task (four a workgroup), as in zh_zip_write_kernel: a slice of an entry's local part (the first
// slice's wave also writes the entry's central directory record), or an archive's end records.  The task is the
// wave's, so the branches are uniform.
__global__ __launch_bounds__(256) void zh_zip_create_kernel(uint8_t* __restrict__ img, const uint8_t* __restrict__ slots,
                                                            const ZhZip64EntryDesc* __restrict__ descs,
                                                            const ZhZip64Task* __restrict__ tasks, uint64_t n_tasks,
                                                            const ZhZip64EndDesc* __restrict__ ends,
                                                            const uint8_t* __restrict__ pool) {
  const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (wave >= n_tasks) return;
  const ZhZip64Task t = tasks[wave];
  if (t.kind == kTaskEnd) {
    const ZhZip64EndDesc e = ends[t.idx];
    write_range(img, t.lo, t.hi, lane, End64Gen{e});
    return;
  }
  const ZhZip64EntryDesc d = descs[t.idx];
  write_range(img, t.lo, t.hi, lane, Local64Gen{d, pool, slots}, d.lh + kLocal64 + d.plen + kLocalExtra, slots, d.src);
  if (t.kind == kTaskFirst) write_range(img, d.cd, d.cd + kCentral64 + d.plen + kCentralExtra, lane, Central64Gen{d, pool});
}

namespace {

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

}  // namespace

extern "C" int zh_zip_create_batch(zh_ctx* ctx, const zh_zip_new_entry* entries, const size_t* first, size_t n_zip,
                                   int level, void** dsts, size_t* dst_lens, int32_t* statuses) {
  if (const int st = writer_checks(ctx, entries, first, n_zip, level < -2 || level > 9 ? ZH_ERR_INVALID_LEVEL : ZH_OK,
                                   dsts, dst_lens, statuses);
      st || !n_zip)
    return st;
  // the tasks name entries and archives in 32 bits (tasks themselves are counted in 64)
  if (first[n_zip] - first[0] >= 0xffffffffull || n_zip >= 0xffffffffull) return ZH_ERR_ARGUMENT;

  // ---- the checks; the non-empty contents of the archives that pass, in processing order, in one device buffer ----
  std::vector<size_t> ok;
  std::vector<const void*> csrc;
  std::vector<size_t> clens;
  std::vector<uint32_t> slot_of(first[n_zip] - first[0], ~0u);  // entry -> its plan buffer
  for (size_t t = 0; t < n_zip; t++) {
    if ((statuses[t] = check_archive64(entries + first[t], first[t + 1] - first[t])) != ZH_OK) continue;
    ok.push_back(t);
    for (size_t i = first[t + 1]; i-- > first[t];) {
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
  tr.mark(ctx, "zip64: upload");

  // ---- compress(contents, level, dfDeflate) and crc32(contents) of every non-empty entry: one plan (:519-530) ----
  std::vector<uint64_t> doff, clen;
  std::vector<int32_t> cst;
  std::vector<uint32_t> crc(csrc.size(), 0);
  if ((st = zhh_compress(ctx, d_src.p, soff, slen, level, ZH_DF_DEFLATE, crc.data(), d_slots, doff, clen, cst)))
    return st;
  tr.mark(ctx, "zip64: compress");
  if (d_src.p) {  // (back to the context's cache before the image is allocated)
    ctx_free(ctx, d_src.p);
    d_src.p = nullptr;
  }

  // ---- the layout: archive t's image is [img_off, + img_len) of one buffer, 256-aligned ----
  std::vector<ZhZip64EntryDesc> descs;
  std::vector<ZhZip64Task> tasks;
  std::vector<ZhZip64EndDesc> ends;
  std::vector<uint8_t> pool;
  std::vector<size_t> done;  // the archives that are written, in order
  std::vector<uint64_t> img_off, img_len;
  uint64_t o = 0;
  for (size_t t : ok) {
    const size_t i0 = first[t], i1 = first[t + 1];
    int ast = ZH_OK;
    uint64_t at = 0, names = 0;  // (offsets inside the archive)
    for (size_t i = i1; i-- > i0 && ast == ZH_OK;) {
      const uint32_t k = slot_of[i - first[0]];
      if (k != ~0u && cst[k] != ZH_OK) ast = cst[k];
      at += kLocal64 + entries[i].path_len + kLocalExtra + (k == ~0u ? 0 : clen[k]);
      names += entries[i].path_len;
    }
    if (ast != ZH_OK) {
      statuses[t] = ast;
      continue;
    }
    const uint64_t cd_size = (uint64_t)(kCentral64 + kCentralExtra) * (i1 - i0) + names;
    done.push_back(t);
    img_off.push_back(o);
    uint64_t cd = o + at;
    for (size_t i = i1; i-- > i0;) {
      const zh_zip_new_entry& e = entries[i];
      const uint32_t k = slot_of[i - first[0]];
      ZhZip64EntryDesc d{};
      d.lh = o;
      d.cd = cd;
      d.src = k == ~0u ? 0 : doff[k];
      d.path = pool.size();
      d.clen = k == ~0u ? 0 : clen[k];
      d.ulen = e.len;
      d.rel = o - img_off.back();
      d.crc = k == ~0u ? 0 : crc[k];
      d.plen = (uint16_t)e.path_len;
      d.method = k == ~0u ? 0 : 8;
      d.time = e.dos_time;
      d.date = e.dos_date;
      pool.insert(pool.end(), (const uint8_t*)e.path, (const uint8_t*)e.path + e.path_len);
      const uint32_t idx = (uint32_t)descs.size();
      descs.push_back(d);
      const uint64_t data_at = o + kLocal64 + e.path_len + kLocalExtra, end = data_at + d.clen;
      uint64_t lo = o;
      for (uint64_t hi = std::min(end, data_at + kSlice);; hi = std::min(end, hi + kSlice)) {
        tasks.push_back({lo, hi, idx, lo == o ? kTaskFirst : kTaskSlice});
        if ((lo = hi) == end) break;
      }
      o = end;
      cd += kCentral64 + e.path_len + kCentralExtra;
    }
    tasks.push_back({cd, cd + kEnd64, (uint32_t)ends.size(), kTaskEnd});
    ends.push_back({cd, (uint64_t)(i1 - i0), cd_size, at});
    img_len.push_back(cd + kEnd64 - img_off.back());
    o = round_up(cd + kEnd64, 256);
  }
  const size_t n_done = done.size();
  if (!n_done) return ZH_OK;

  // ---- descriptors, tasks, end records and names in one upload ----
  DevBuf d_meta, d_img;
  std::vector<uint64_t> moff;
  if ((st = zhh_upload_spans(ctx, {{descs.data(), descs.size() * sizeof(ZhZip64EntryDesc)},
                                   {tasks.data(), tasks.size() * sizeof(ZhZip64Task)},
                                   {ends.data(), ends.size() * sizeof(ZhZip64EndDesc)}, {pool.data(), pool.size()}},
                             d_meta, moff)))
    return st;
  if (dev_alloc(ctx, d_img, o + 256) != hipSuccess) return ZH_ERR_NOMEM;
  tr.mark(ctx, "zip64: layout");

  uint8_t* const img = d_img.p;
  const uint8_t *const mp = d_meta.p, *const slots = d_slots.p;
  constexpr uint64_t kGridTasks = 4ull << 22;  // tasks a launch: 2^22 workgroups
  for (uint64_t t0 = 0; t0 < tasks.size(); t0 += kGridTasks) {
    const uint64_t nt = std::min<uint64_t>(kGridTasks, tasks.size() - t0);
    hipLaunchKernelGGL(zh_zip_create_kernel, dim3((uint32_t)((nt + 3) / 4)), dim3(256), 0, ctx->stream, img,
                       slots, reinterpret_cast<const ZhZip64EntryDesc*>(mp + moff[0]),
                       reinterpret_cast<const ZhZip64Task*>(mp + moff[1]) + t0, nt,
                       reinterpret_cast<const ZhZip64EndDesc*>(mp + moff[2]), mp + moff[3]);
    ZH_HIP(ctx, hipGetLastError());
  }
  tr.mark(ctx, "zip64: write");

  if ((st = writer_hand_out(ctx, d_img.p, done, img_off, img_len, std::vector<int32_t>(n_done, ZH_OK), dsts,
                            dst_lens, statuses)))
    return st;
  tr.mark(ctx, "zip64: download");
  return ZH_OK;
}
