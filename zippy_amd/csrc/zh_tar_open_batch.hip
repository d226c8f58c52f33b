// Reading tarballs: extractAll (src/zippy/tarballs.nim:26-124) without its file-system half, for many images a call.
// The host classifies the images by length and magic bytes; every gzip member of the call is decoded by ONE sized
// uncompress plan whose outputs stay in HBM, the plain images are uploaded next to them.  The ustar header walk of
// tarballs.nim:61-124 -- serial by nature: a header's position is the sum of the sizes before it -- runs in parallel:
//   zh_tar_next_kernel    every 512-byte block of every image is read as if it were a header: next[b]
//   zh_walk_double_kernel the blocks reachable from an image's block 0 ARE its headers: pointer doubling (zh_walk.h)
//   zh_walk_scan_*        a prefix sum over the marks: every header's ordinal in walk order, the list of headers
//   zh_tar_parse_kernel   one wave per header: fields, the joined path, the checks, one fixed-size record
//   zh_tar_reduce_kernel  per tarball: the first header in walk order that failed is the tarball's status
// The host builds the zh_tar_readers from the records; it parses no header byte itself.
#include "zh_tar_dev.h"

namespace {

// One header that tarballs.nim:61-124 looks at (48 bytes).  `reported`: an entry of the reader (typeflags 0, \0, 5,
// 2 of an active header); the other fields mean something only then.  The path is the 256-byte pool slot of the
// header's ordinal (path_off = 256 * ordinal), or -- a pending long name -- image bytes [path_off, + path_len).
struct ZhTarRec {
  uint64_t offset, size, path_off, path_len;
  int64_t mtime;
  uint32_t mode;
  uint8_t typeflag, link_len, reported, path_in_image;
};

// tarballs.nim:5-23 parseTarOctInt over the n bytes that start `shift` bytes into the 16 bytes (lo, hi): the first
// run of decimal digits, read as octal; a digit 8 or 9 in it is an error (-> false)
__device__ __forceinline__ bool tar_octal(uint64_t lo, uint64_t hi, uint32_t shift, uint32_t n, uint64_t* out) {
  uint64_t v = 0;
  uint32_t state = 0;  // 0 before the run, 1 inside, 2 behind it
  bool ok = true;
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t at = shift + k;
    const uint32_t c = (uint32_t)((at < 8 ? lo >> (8 * at) : hi >> (8 * (at - 8))) & 0xffu);
    const bool digit = c >= '0' && c <= '9';
    if (state == 0 && digit) state = 1;
    if (state == 1) {
      if (digit) {
        ok = ok && c <= '7';
        v = v * 8 + (c - '0');
      } else {
        state = 2;
      }
    }
  }
  *out = v;
  return ok;
}

// the size field (bytes 124-134) of the header at h, read with three aligned 32-bit loads
__device__ __forceinline__ bool header_size(const uint8_t* __restrict__ h, uint64_t* size) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(h + 124);
  return tar_octal((uint64_t)w[0] | ((uint64_t)w[1] << 32), (uint64_t)w[2], 0, 11, size);
}

}  // namespace

// next[b] for every node b: the node of the header that follows if block b is a header -- END when the size field
// does not parse, when the entry runs past the image, when b is a trailing partial block, and for END itself.
// mark[b] = 1 for the first block of every tarball.  Of a block, one 128-byte line in four is touched.
__global__ __launch_bounds__(256) void zh_tar_next_kernel(const ZhTarImg* __restrict__ imgs, uint32_t n_img,
                                                          uint32_t n_nodes, uint32_t* __restrict__ jump,
                                                          uint32_t* __restrict__ mark) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n_nodes) return;
  const ZhTarImg g = imgs[find_img(imgs, n_img, b)];
  const uint32_t end = g.blk0 + g.nblk;
  uint32_t nx = end;
  if (b != end) {
    const uint64_t pos = (uint64_t)(b - g.blk0) * 512;
    uint64_t size;
    if (pos + 512 <= g.len && header_size(g.data + pos, &size) && pos + 512 + size <= g.len) {
      const uint64_t nk = (uint64_t)(b - g.blk0) + 1 + ((size + 511) >> 9);
      if (nk < g.nblk) nx = g.blk0 + (uint32_t)nk;
    }
  }
  jump[b] = nx;
  mark[b] = b == g.blk0 && b != end ? 1u : 0u;
}

// One wave per header, in walk order (h = its ordinal in the call, list[h] its node).  The lanes load the header 8
// bytes each; string fields end at the first zero byte of their range (ballot + shuffle), the octal fields are read
// from the two lanes that hold them.  The header's own status follows the reference's order: the block is whole
// (tarballs.nim:62-63), mode / size / mtime parse (:65-67), the contents are there (:77-78), then -- for a header
// that has a name or a pending long name (:80) -- the path is safe (:87) and the type is known (:89-119).
// A long name is pending for header i when header i - 1 is an 'L' block of size > 0 that was itself active: that has
// a name, or -- the look-back along a run of 'L' blocks with empty names -- a pending long name of its own.
__global__ __launch_bounds__(256) void zh_tar_parse_kernel(const ZhTarImg* __restrict__ imgs, uint32_t n_img,
                                                           const uint32_t* __restrict__ ord,
                                                           const uint32_t* __restrict__ list, uint32_t n_hdr,
                                                           ZhTarRec* __restrict__ recs, uint32_t* __restrict__ pool,
                                                           int32_t* __restrict__ hstat) {
  const uint32_t h = blockIdx.x * 4 + (threadIdx.x >> 6), lane = zh_lane();
  if (h >= n_hdr) return;
  const uint32_t node = list[h];
  const ZhTarImg g = imgs[find_img(imgs, n_img, node)];
  const uint32_t first = ord[g.blk0];  // the ordinal of the tarball's first header
  const uint64_t pos = (uint64_t)(node - g.blk0) * 512;
  ZhTarRec rec{};
  int32_t status = ZH_OK;
  if (pos + 512 > g.len) {  // a trailing partial block
    status = ZH_ERR_ARCHIVE_EOF;
  } else {
    const uint8_t* __restrict__ hdr = g.data + pos;
    const uint64_t w = reinterpret_cast<const uint64_t*>(hdr)[lane];
    uint32_t zm = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) zm |= ((w >> (8 * k)) & 0xffu) == 0 ? 1u << k : 0u;
    const uint32_t name_len = field_len(zm, lane, 0, 100), link_len = field_len(zm, lane, 157, 100);
    const uint32_t magic_len = field_len(zm, lane, 257, 6);
    uint32_t prefix_len = field_len(zm, lane, 345, 155);
    const bool ustar = magic_len == 5 && ((__shfl(w, 32) >> 8) & 0xffffffffffull) == 0x7261747375ull;
    if (!ustar) prefix_len = 0;
    uint64_t mode, size, mtime;
    const bool ok_mode = tar_octal(__shfl(w, 12), __shfl(w, 13), 4, 7, &mode);
    const bool ok_size = tar_octal(__shfl(w, 15), __shfl(w, 16), 4, 11, &size);
    const bool ok_mtime = tar_octal(__shfl(w, 17), __shfl(w, 18), 0, 11, &mtime);
    const uint32_t typeflag = (uint32_t)(__shfl(w, 19) >> 32) & 0xffu;

    // is a long name pending?  (every lane reads the same bytes: the loop is uniform)
    bool pending = false;
    uint64_t long_at = 0, long_len = 0;
    for (uint32_t i = h; i > first; i--) {
      const uint64_t p = (uint64_t)(list[i - 1] - g.blk0) * 512;
      uint64_t psize = 0;
      if (g.data[p + 156] != 'L' || !header_size(g.data + p, &psize) || psize == 0) break;
      if (i == h) {
        long_at = p + 512;
        long_len = psize;
      }
      if (g.data[p] != 0) {
        pending = true;
        break;
      }
    }

    if (!ok_mode || !ok_size || !ok_mtime) {
      status = ZH_ERR_TAR_NUMBER;
    } else if (pos + 512 + size > g.len) {
      status = ZH_ERR_ARCHIVE_EOF;
    } else if (name_len || pending) {
      bool unsafe = false;
      if (pending) {  // the long name, 512 bytes a step; a lane looks at the 8 positions of its bytes
        const uint8_t* __restrict__ q = g.data + long_at;
        for (uint64_t c = 0; c < long_len && !unsafe; c += 512) {
          const uint64_t o = c + lane * 8;
          uint64_t lo = o < long_len ? *reinterpret_cast<const uint64_t*>(q + o) : 0ull;
          uint64_t hi = o + 8 < long_len ? (uint64_t) * reinterpret_cast<const uint32_t*>(q + o + 8) : 0ull;
          const uint64_t left = o < long_len ? long_len - o : 0;  // bytes of the name from o on; the rest reads as 0
          if (left < 8) lo &= (1ull << (8 * left)) - 1ull;
          if (left < 12) hi &= left > 8 ? (1ull << (8 * (left - 8))) - 1ull : 0ull;
          bool bad = false;
#pragma unroll
          for (uint32_t k = 0; k < 8; k++) {
            const uint32_t x = (uint32_t)(k ? (lo >> (8 * k)) | (hi << (64 - 8 * k)) : lo);
            bad = bad || (k < left && unsafe_at(x, o + k));
          }
          unsafe = __ballot(bad) != 0;
        }
        rec.path_off = long_at;
        rec.path_len = long_len;
        rec.path_in_image = 1;
      } else {  // prefix / name with the rules of std/os `/`; a lane makes 4 bytes of the joined path
        const bool hs = prefix_len && hdr[345 + prefix_len - 1] == '/', ts = hdr[0] == '/';
        const uint32_t sep = prefix_len && !hs && !ts ? 1u : 0u, skip = hs && ts ? 1u : 0u;
        const uint32_t total = prefix_len + sep + name_len - skip;
        auto at = [&](uint32_t j) -> uint32_t {
          if (j >= total) return 0u;
          if (j < prefix_len) return hdr[345 + j];
          j -= prefix_len;
          if (sep) {
            if (j == 0) return '/';
            j--;
          }
          return hdr[skip + j];
        };
        uint32_t c[7];
#pragma unroll
        for (uint32_t k = 0; k < 7; k++) c[k] = at(lane * 4 + k);
        bool bad = false;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++)
          bad = bad || (lane * 4 + k < total &&
                        unsafe_at(c[k] | (c[k + 1] << 8) | (c[k + 2] << 16) | (c[k + 3] << 24), lane * 4 + k));
        unsafe = __ballot(bad) != 0;
        pool[(uint64_t)h * 64 + lane] = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
        rec.path_off = (uint64_t)h * 256;
        rec.path_len = total;
      }
      if (unsafe) {
        status = ZH_ERR_UNSAFE_PATH;
      } else if (typeflag == '0' || typeflag == 0 || typeflag == '5' || typeflag == '2') {
        rec.reported = 1;
        rec.offset = pos + 512;
        rec.size = size;
        rec.mtime = (int64_t)mtime;
        rec.mode = (uint32_t)mode;
        rec.typeflag = (uint8_t)typeflag;
        rec.link_len = (uint8_t)link_len;
      } else if (typeflag == 'g' || typeflag == 'x' || (typeflag >= 'A' && typeflag <= 'Z')) {
        // a long name ('L'), extended headers and vendor types: nothing to report
      } else {
        status = ZH_ERR_TAR_HEADER_TYPE;
      }
    }
  }
  if (lane == 0) {
    recs[h] = rec;
    hstat[h] = status;
  }
}

extern "C" int zh_tar_open_batch(zh_ctx* ctx, const void* const* images, const size_t* lens, size_t n_tar,
                                 zh_tar_reader** readers, int32_t* statuses) {
  if (const int e = reader_checks(ctx, images, lens, n_tar, readers, statuses)) return e;
  if (!n_tar) return ZH_OK;

  // ---- classify: lengths and magic bytes only (tarballs.nim:43-54, gzip.nim:10-11) ----
  std::vector<size_t> gz, plain;
  for (size_t t = 0; t < n_tar; t++) {
    const uint8_t* s = (const uint8_t*)images[t];
    if (lens[t] < 2 || (s[0] == 31 && s[1] == 139 && lens[t] < 18))
      statuses[t] = ZH_ERR_INVALID_BUFFER;
    else if (s[0] == 31 && s[1] == 139)
      gz.push_back(t);
    else
      plain.push_back(t);
  }
  if (gz.empty() && plain.empty()) return ZH_OK;
  ZH_HIP(ctx, hipSetDevice(ctx->device));
  Trace tr;
  int st;

  // ---- one upload, one decode (zh_tar_dev.h) ----
  TarStage stage;
  if ((st = tar_stage(ctx, images, lens, plain, gz, statuses, tr, "tar open: upload", "tar open: decode", stage)))
    return st;
  const std::vector<TarWalk>& walk = stage.walk;
  const size_t n_walk = walk.size();
  if (!n_walk) return ZH_OK;

  // ---- the walk (zh_walk.h) ----
  std::vector<ZhTarImg> imgs;
  uint32_t N = 0, rounds = 0;
  if ((st = tar_nodes(walk, imgs, &N, &rounds))) return st;
  DevBuf d_imgs;
  std::vector<uint64_t> ioff;
  if ((st = zhh_upload_spans(ctx, {{imgs.data(), n_walk * sizeof(ZhTarImg)}}, d_imgs, ioff))) return st;
  Walk w;
  if ((st = walk_alloc(ctx, w, N))) return st;
  // (plain pointers for the launches: a launch must not take a DevBuf, or the Walk that holds one, along)
  const ZhTarImg* const dimgs = reinterpret_cast<const ZhTarImg*>(d_imgs.p);
  uint32_t *const j0 = w.j0, *const mark = w.mark;
  const uint32_t *const ord = w.ord, *const list = w.list;
  const dim3 wg(256);
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(zh_tar_next_kernel, dim3((N + 255) / 256), wg, 0, s, dimgs, (uint32_t)n_walk, N, j0, mark);
  walk_double(w, rounds, s);
  walk_scan(w, s);
  uint32_t n_hdr = 0;
  if ((st = walk_count(ctx, w, &n_hdr))) return st;
  tr.mark(ctx, "tar open: reach + scan");

  // results: records, path pool, the tarballs' header ranges and statuses come back; the headers' statuses stay
  TarResults<ZhTarRec> res;
  if ((st = tar_results(ctx, stage, w, dimgs, n_walk, n_hdr,
                        [&](ZhTarRec* d_recs, uint32_t* d_pool, int32_t* d_hstat) {
                          hipLaunchKernelGGL(zh_tar_parse_kernel, dim3((n_hdr + 3) / 4), wg, 0, s, dimgs,
                                             (uint32_t)n_walk, ord, list, n_hdr, d_recs, d_pool, d_hstat);
                        },
                        res)))
    return st;
  tr.mark(ctx, "tar open: parse + reduce");

  // ---- the decoded images of the tarballs that opened ----
  if ((st = tar_fetch(ctx, stage, res.tstat))) return st;
  tr.mark(ctx, "tar open: download");

  // ---- the readers, from the records ----
  std::vector<zh_tar_reader*> made(n_walk, nullptr);
  CloseAll close_made{made};
  for (size_t k = 0; k < n_walk; k++) {
    if (res.tstat[k] != ZH_OK) continue;
    const uint8_t* data;
    zh_tar_reader* r = made[k] = tar_reader_of(stage, k, images, &data);
    if (!r) return ZH_ERR_NOMEM;
    for (uint32_t i = res.ranges[2 * k]; i < res.ranges[2 * k + 1]; i++) {
      const ZhTarRec& e = res.recs[i];
      if (!e.reported) continue;
      const char* path = (const char*)(e.path_in_image ? data : res.pool) + e.path_off;
      if (zh_tar_reader_add(r, path, (size_t)e.path_len, (const char*)data + e.offset - 512 + 157, e.link_len,
                            (char)e.typeflag, e.mode, e.mtime, e.offset, e.size) != ZH_OK)
        return ZH_ERR_NOMEM;
    }
  }
  close_made.armed = false;
  for (size_t k = 0; k < n_walk; k++) {
    readers[walk[k].t] = made[k];
    statuses[walk[k].t] = res.tstat[k];
  }
  return ZH_OK;
}
