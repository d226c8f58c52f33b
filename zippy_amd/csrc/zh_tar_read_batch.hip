// Tarball.open of the v1 API (src/zippy/tarballs_v1.nim:66-157 openStreamImpl), for many images a call.  The host
// classifies the images by the caller's format, their lengths and their first two bytes (:79-96); every gzip image of
// the call is decoded by ONE sized uncompress plan whose outputs stay in HBM, the plain images are uploaded next to
// them (zh_tar_dev.h).  The header loop of :98-157 -- serial by nature: a header's position is the sum of the sizes
// before it -- runs in parallel:
//   zh_tarv_next_kernel   every 512-byte block of every image is read as if the loop stood on it: next[b]
//   zh_walk_double_kernel the blocks reachable from an image's block 0 ARE the blocks the loop stands on (zh_walk.h)
//   zh_tarv_select_kernel of those, the ones the host needs a record for: a name, or a trailing partial block
//   zh_walk_scan_*        a prefix sum over them: every header's ordinal in walk order, the list of headers
//   zh_tarv_parse_kernel  one wave per header: the three strict numbers, the key, the checks, one fixed-size record
//   zh_tar_reduce_kernel  per tarball: the first header in walk order that failed is the tarball's status
// The host builds the tables from the keys and hands them out as zh_tar_readers; it parses no header byte itself.
#include <string>
#include <unordered_map>

#include "zh_tar_dev.h"

namespace {

// One named header (32 bytes).  `reported`: typeflag '0', '\0' (-> '0') or '5'; the other fields mean something only
// then, and are 0 for a directory.  The key is the 256-byte pool slot of the header's ordinal.
struct ZhTarvRec {
  uint64_t offset, size;
  int64_t mtime;
  uint32_t mode;
  uint16_t key_len;
  uint8_t typeflag, reported;
};

// strutils.parseOctInt over the n bytes that start `shift` bytes into the 16 bytes (lo, hi): an optional 0o / 0O when
// a byte follows it, then digits 0-7 and underscores; true when that is all of the slice and a digit was among them
__device__ __forceinline__ bool strict_octal(uint64_t lo, uint64_t hi, uint32_t shift, uint32_t n, uint64_t* out) {
  auto at = [&](uint32_t k) -> uint32_t {
    const uint32_t a = shift + k;
    return (uint32_t)((a < 8 ? lo >> (8 * a) : hi >> (8 * (a - 8))) & 0xffu);
  };
  const uint32_t start = n > 2 && at(0) == '0' && (at(1) == 'o' || at(1) == 'O') ? 2u : 0u;
  uint64_t v = 0;
  bool scanning = true, digit = false;
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t c = at(k);
    const bool d = c >= '0' && c <= '7';
    if (k >= start) {
      if (scanning && d) {
        v = (v << 3) | (c - '0');
        digit = true;
      }
      scanning = scanning && (d || c == '_');
    }
  }
  *out = v;
  return scanning && digit;
}

}  // namespace

// next[b] for every node b, as tarballs_v1.nim:99-157 goes on from block b: b + 1 behind a header without a name
// (:109-110, its size field is not read); behind a named one the block after its padded contents -- END when the
// size field does not parse, when the contents reach the image's end, when b is a trailing partial block, and for
// END itself.  rec[b] = 1 for a block the host needs a record for: a name, or partial.  mark[b] = 1 for the first
// block of every tarball.  Of a block, bytes 0 and 124-135 are read: two of its four 128-byte lines.
__global__ __launch_bounds__(256) void zh_tarv_next_kernel(const ZhTarImg* __restrict__ imgs, uint32_t n_img,
                                                           uint32_t n_nodes, uint32_t* __restrict__ jump,
                                                           uint32_t* __restrict__ mark, uint8_t* __restrict__ rec) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n_nodes) return;
  const ZhTarImg g = imgs[find_img(imgs, n_img, b)];
  const uint32_t end = g.blk0 + g.nblk;
  uint32_t nx = end;
  uint8_t r = 0;
  if (b != end) {
    const uint64_t idx = b - g.blk0, pos = idx * 512;
    if (pos + 512 > g.len) {
      r = 1;
    } else if (g.data[pos] == 0) {
      nx = b + 1;
    } else {
      r = 1;
      const uint32_t* w = reinterpret_cast<const uint32_t*>(g.data + pos + 124);
      uint64_t size;
      if (strict_octal((uint64_t)w[0] | ((uint64_t)w[1] << 32), (uint64_t)w[2], 0, 11, &size)) {
        const uint64_t nk = idx + 1 + ((size + 511) >> 9);
        if (nk < g.nblk) nx = g.blk0 + (uint32_t)nk;
      }
    }
  }
  jump[b] = nx;
  rec[b] = r;
  mark[b] = b == g.blk0 && b != end ? 1u : 0u;
}

// After the doubling: of the reachable blocks, keep the marks of those that get a record.  A run of zero blocks costs
// its marks and nothing else.
__global__ __launch_bounds__(256) void zh_tarv_select_kernel(uint32_t* __restrict__ mark,
                                                             const uint8_t* __restrict__ rec, uint32_t n_nodes) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b < n_nodes) mark[b] &= rec[b];
}

// One wave per listed header, in walk order (h = its ordinal in the call, list[h] its node).  The lanes load the
// header 8 bytes each; string fields end at the first zero byte of their range (ballot + shuffle), the numbers are
// read from the two lanes that hold them.  The header's status follows the reference's order: the block is whole
// (tarballs_v1.nim:100), size and mtime parse (:113-125), mode parses (:127-132), the contents are there (:139).
// The key is (prefix / name).toUnixPath(), the prefix counting only behind the six bytes "ustar\0" (:133-137).
__global__ __launch_bounds__(256) void zh_tarv_parse_kernel(const ZhTarImg* __restrict__ imgs, uint32_t n_img,
                                                            const uint32_t* __restrict__ list, uint32_t n_hdr,
                                                            ZhTarvRec* __restrict__ recs, uint32_t* __restrict__ pool,
                                                            int32_t* __restrict__ hstat) {
  const uint32_t h = blockIdx.x * 4 + (threadIdx.x >> 6), lane = zh_lane();
  if (h >= n_hdr) return;
  const uint32_t node = list[h];
  const ZhTarImg g = imgs[find_img(imgs, n_img, node)];
  const uint64_t pos = (uint64_t)(node - g.blk0) * 512;
  ZhTarvRec rec{};
  int32_t status = ZH_OK;
  if (pos + 512 > g.len) {  // a trailing partial block
    status = ZH_ERR_TAR_EOF;
  } else {
    const uint8_t* __restrict__ hdr = g.data + pos;
    const uint64_t w = reinterpret_cast<const uint64_t*>(hdr)[lane];
    uint32_t zm = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) zm |= ((w >> (8 * k)) & 0xffu) == 0 ? 1u << k : 0u;
    const uint32_t name_len = field_len(zm, lane, 0, 100);
    uint32_t prefix_len = field_len(zm, lane, 345, 155);
    // header[257 ..< 263] == "ustar\0": the NUL is part of the compare
    if (((__shfl(w, 32) >> 8) & 0xffffffffffffull) != 0x007261747375ull) prefix_len = 0;
    uint64_t mode, size, mtime;
    const bool ok_mode = strict_octal(__shfl(w, 12), __shfl(w, 13), 4, 6, &mode);
    const bool ok_size = strict_octal(__shfl(w, 15), __shfl(w, 16), 4, 11, &size);
    const bool ok_mtime = strict_octal(__shfl(w, 17), __shfl(w, 18), 0, 11, &mtime);
    const uint32_t typeflag = (uint32_t)(__shfl(w, 19) >> 32) & 0xffu;

    if (!ok_size || !ok_mtime) {
      status = ZH_ERR_TAR_OPEN;
    } else if (!ok_mode) {
      status = ZH_ERR_TAR_OPEN_MODE;
    } else if (pos + 512 + size > g.len) {
      status = ZH_ERR_TAR_EOF;
    } else if (typeflag == '0' || typeflag == 0 || typeflag == '5') {
      // prefix / name with the rules of std/os `/`, then every \ as /; a lane makes 4 bytes of the key
      const bool hs = prefix_len && hdr[345 + prefix_len - 1] == '/', ts = hdr[0] == '/';
      const uint32_t sep = prefix_len && !hs && !ts ? 1u : 0u, skip = hs && ts ? 1u : 0u;
      const uint32_t total = prefix_len + sep + name_len - skip;
      auto at = [&](uint32_t j) -> uint32_t {
        if (j >= total) return 0u;
        uint32_t c;
        if (j < prefix_len) {
          c = hdr[345 + j];
        } else if (sep && j == prefix_len) {
          c = '/';
        } else {
          c = hdr[skip + j - prefix_len - sep];
        }
        return c == '\\' ? (uint32_t)'/' : c;
      };
      uint32_t word = 0;
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) word |= at(lane * 4 + k) << (8 * k);
      pool[(uint64_t)h * 64 + lane] = word;
      rec.reported = 1;
      rec.key_len = (uint16_t)total;
      if (typeflag == '5') {  // TarballEntry(kind: ekDirectory): nothing else
        rec.typeflag = '5';
      } else {
        rec.typeflag = '0';
        rec.offset = pos + 512;
        rec.size = size;
        rec.mtime = (int64_t)mtime;
        rec.mode = (uint32_t)mode;
      }
    }
  }
  if (lane == 0) {
    recs[h] = rec;
    hstat[h] = status;
  }
}

extern "C" int zh_tar_read_batch(zh_ctx* ctx, const void* const* images, const size_t* lens, const int32_t* formats,
                                 size_t n_tar, zh_tar_reader** readers, int32_t* statuses) {
  if (const int e = reader_checks(ctx, images, lens, n_tar, readers, statuses)) return e;
  for (size_t t = 0; formats && t < n_tar; t++)
    if (formats[t] < ZH_TF_DETECT || formats[t] > ZH_TF_GZIP) return ZH_ERR_ARGUMENT;
  if (!n_tar) return ZH_OK;

  // ---- classify: the format, lengths and the first two bytes only (tarballs_v1.nim:79-96, gzip.nim:10-11) ----
  std::vector<size_t> gz, plain, empty;
  for (size_t t = 0; t < n_tar; t++) {
    const uint8_t* s = (const uint8_t*)images[t];
    int fmt = formats ? formats[t] : ZH_TF_DETECT;
    if (fmt == ZH_TF_DETECT) {
      // (the reference indexes past the string for 0 bytes, and for 1 byte that is 0x1F: a Defect there)
      if (!lens[t] || (s[0] == 0x1f && (lens[t] < 2 || s[1] != 0x8b))) {
        statuses[t] = ZH_ERR_TAR_FORMAT;
        continue;
      }
      fmt = s[0] == 0x1f ? ZH_TF_GZIP : ZH_TF_UNCOMPRESSED;
    }
    if (fmt == ZH_TF_GZIP) {
      if (lens[t] < 18)
        // gzip.nim:10-11, the decoder's first check (zh_inflate.hip's unwrap kernel: `len < 18` under ZH_DF_GZIP);
        // tests/tar_read_cases.py holds these images to zh_uncompress_batch's status, so the two cannot drift apart
        statuses[t] = ZH_ERR_INVALID_BUFFER;
      else
        gz.push_back(t);
    } else if (lens[t]) {
      plain.push_back(t);
    } else {
      empty.push_back(t);  // the loop of :99 never runs
    }
  }
  std::vector<zh_tar_reader*> made_empty(empty.size(), nullptr);
  CloseAll close_empty{made_empty};
  for (size_t k = 0; k < empty.size(); k++)
    if (!(made_empty[k] = zh_tar_reader_new(nullptr, images[empty[k]], 0))) return ZH_ERR_NOMEM;
  auto hand_out_empty = [&]() {
    for (size_t k = 0; k < empty.size(); k++) readers[empty[k]] = made_empty[k];
    close_empty.armed = false;
    return ZH_OK;
  };
  if (gz.empty() && plain.empty()) return hand_out_empty();
  ZH_HIP(ctx, hipSetDevice(ctx->device));
  Trace tr;
  int st;

  // ---- one upload, one decode (zh_tar_dev.h) ----
  TarStage stage;
  if ((st = tar_stage(ctx, images, lens, plain, gz, statuses, tr, "tar read: upload", "tar read: decode", stage)))
    return st;
  const std::vector<TarWalk>& walk = stage.walk;
  const size_t n_walk = walk.size();
  if (!n_walk) return hand_out_empty();

  // ---- the walk (zh_walk.h); behind its scratch a byte a node for "gets a record" ----
  std::vector<ZhTarImg> imgs;
  uint32_t N = 0, rounds = 0;
  if ((st = tar_nodes(walk, imgs, &N, &rounds))) return st;
  DevBuf d_imgs;
  std::vector<uint64_t> ioff;
  if ((st = zhh_upload_spans(ctx, {{imgs.data(), n_walk * sizeof(ZhTarImg)}}, d_imgs, ioff))) return st;
  Walk w;
  if ((st = walk_alloc(ctx, w, N, N))) return st;
  // (plain pointers for the launches: a launch must not take a DevBuf, or the Walk that holds one, along)
  const ZhTarImg* const dimgs = reinterpret_cast<const ZhTarImg*>(d_imgs.p);
  uint32_t *const j0 = w.j0, *const mark = w.mark;
  const uint32_t* const list = w.list;
  uint8_t* const rec = w.extra;
  const dim3 node_grid((N + 255) / 256), wg(256);
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(zh_tarv_next_kernel, node_grid, wg, 0, s, dimgs, (uint32_t)n_walk, N, j0, mark, rec);
  walk_double(w, rounds, s);
  hipLaunchKernelGGL(zh_tarv_select_kernel, node_grid, wg, 0, s, mark, (const uint8_t*)rec, N);
  walk_scan(w, s);
  uint32_t n_hdr = 0;  // the named headers
  if ((st = walk_count(ctx, w, &n_hdr))) return st;
  tr.mark(ctx, "tar read: reach + scan");

  // results: records, key pool, the tarballs' header ranges and statuses come back; the headers' statuses stay
  TarResults<ZhTarvRec> res;
  if ((st = tar_results(ctx, stage, w, dimgs, n_walk, n_hdr,
                        [&](ZhTarvRec* d_recs, uint32_t* d_pool, int32_t* d_hstat) {
                          hipLaunchKernelGGL(zh_tarv_parse_kernel, dim3((n_hdr + 3) / 4), wg, 0, s, dimgs,
                                             (uint32_t)n_walk, list, n_hdr, d_recs, d_pool, d_hstat);
                        },
                        res)))
    return st;
  const ZhTarvRec* const recs = res.recs;
  const char* const keys = (const char*)res.pool;
  const uint32_t* const ranges = res.ranges;
  const int32_t* const tstat = res.tstat;
  tr.mark(ctx, "tar read: parse + reduce");

  // ---- the decoded images of the tarballs that opened ----
  if ((st = tar_fetch(ctx, stage, tstat))) return st;
  tr.mark(ctx, "tar read: download");

  // ---- the tables, from the keys: contents[key] = entry replaces an equal key's value and keeps its place ----
  std::vector<zh_tar_reader*> made(n_walk, nullptr);
  CloseAll close_made{made};
  try {
    std::unordered_map<std::string, size_t> place;
    std::vector<uint32_t> table;  // ordinals, in the table's order
    for (size_t k = 0; k < n_walk; k++) {
      if (tstat[k] != ZH_OK) continue;
      const uint8_t* data;
      zh_tar_reader* r = made[k] = tar_reader_of(stage, k, images, &data);
      if (!r) return ZH_ERR_NOMEM;
      place.clear();
      table.clear();
      for (uint32_t i = ranges[2 * k]; i < ranges[2 * k + 1]; i++) {
        if (!recs[i].reported) continue;
        const auto at = place.emplace(std::string(keys + (size_t)i * 256, recs[i].key_len), table.size());
        if (at.second)
          table.push_back(i);
        else
          table[at.first->second] = i;
      }
      for (uint32_t i : table) {
        const ZhTarvRec& e = recs[i];
        if (zh_tar_reader_add(r, keys + (size_t)i * 256, e.key_len, "", 0, (char)e.typeflag, e.mode, e.mtime, e.offset,
                              e.size) != ZH_OK)
          return ZH_ERR_NOMEM;
      }
    }
  } catch (...) {
    return ZH_ERR_NOMEM;
  }
  close_made.armed = false;
  for (size_t k = 0; k < n_walk; k++) {
    readers[walk[k].t] = made[k];
    statuses[walk[k].t] = tstat[k];
  }
  return hand_out_empty();
}
