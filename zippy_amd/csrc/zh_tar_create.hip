// Writing tarballs: writeTarball (src/zippy/tarballs_v1.nim:203-270) for many in-memory tarballs at once.
// The host checks the entries, splits their paths and lays every image out in one device buffer; the entries'
// contents go straight to their final offsets through the pinned staging (zhh_upload_slices); zh_tar_header_kernel
// writes every other byte of the images -- headers, the zero padding behind the contents, the trailers --; for
// .tar.gz the images are then compressed in place as one batch (compress(data, level, dfGzip), :269).
#include <unordered_set>

#include "zh_gather.h"
#include "zh_host.h"

namespace {

// One entry's header, for the kernel (48 bytes).  hdr: image offset of the 512-byte header, the contents follow at
// hdr + 512.  path: offset of the entry's path in the name pool; head = path[0, head_len), tail = path[tail_at, +
// tail_len) (std/os splitPath: head is a prefix of the path, tail a suffix).
struct ZhTarHdrDesc {
  uint64_t hdr, len, mtime, path;
  uint32_t tail_at;
  uint16_t head_len, tail_len;
  uint32_t kind, pad;
};

constexpr uint64_t kOct11 = 1ull << 33;  // 8^11: toOct(x, 11) keeps every digit below this

// tarballs_v1.nim:229-247: the header's byte b, with the checksum field (148-155) as eight spaces
__device__ __forceinline__ uint32_t header_byte(const ZhTarHdrDesc& d, const uint8_t* __restrict__ pool, uint32_t b) {
  // toOct(x, n) ends at byte `end`: the digit of b is x >> 3 * (end - 1 - b)
  auto oct = [](uint64_t x, uint32_t b, uint32_t end) { return (uint32_t)('0' + ((x >> (3 * (end - 1 - b))) & 7)); };
  if (b < 100) return b < d.tail_len ? pool[d.path + d.tail_at + b] : 0u;  // tail, NUL-padded
  if (b < 108) return b < 106 ? (b < 103 ? '0' : '7') : b == 106 ? ' ' : 0u;  // "000777 \0"
  if (b < 124) {                                                              // uid, gid: toOct(0, 6) & " \0"
    const uint32_t k = (b - 108) & 7;
    return k < 6 ? '0' : k == 6 ? ' ' : 0u;
  }
  if (b < 136) return b == 135 ? ' ' : oct(d.len, b, 135);    // toOct(len, 11) & ' '
  if (b < 148) return b == 147 ? ' ' : oct(d.mtime, b, 147);  // toOct(mtime, 11) & ' '
  if (b < 156) return ' ';                                    // checksum: eight spaces while summing
  if (b == 156) return d.kind;
  if (b < 257) return 0;
  if (b < 263) return (uint32_t)(0x7261747375ull >> (8 * (b - 257))) & 0xffu;  // "ustar\0"
  if (b < 265) return '0';                                                      // toOct(0, 2)
  if (b < 329) return 0;
  if (b < 345) {  // devmajor, devminor: toOct(0, 6) & "\0 "
    const uint32_t k = (b - 329) & 7;
    return k < 6 ? '0' : k == 6 ? 0u : ' ';
  }
  if (b < 500) return b - 345 < d.head_len ? pool[d.path + (b - 345)] : 0u;  // head, NUL-padded
  return 0;
}

}  // namespace

// One wave per entry, then one wave per tarball.  Every image byte outside the contents is written exactly once,
// 16 bytes a lane:
//  - entry waves: lanes 0-31 build the 32 chunks of the header; the checksum (the unsigned sum of the 512 bytes,
//    :249-255) is a wave reduction, and lane 9 -- the chunk of bytes 144-159 -- puts toOct(sum, 6) & '\0' into
//    148-154 before it stores.  Lanes 32-63 zero [hdr + 512 + len, next header), at most 32 chunks; the chunk that
//    straddles the end of the contents is loaded, its bytes past the contents cleared, and stored by the same lane.
//  - tarball waves: the 1024-byte trailer (:261), one chunk a lane.
__global__ __launch_bounds__(256) void zh_tar_header_kernel(uint8_t* __restrict__ img,
                                                            const ZhTarHdrDesc* __restrict__ descs, uint64_t n_entries,
                                                            const uint64_t* __restrict__ trailers, uint64_t n_trailers,
                                                            const uint8_t* __restrict__ pool) {
  const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (wave >= n_entries) {
    if (wave - n_entries >= n_trailers) return;
    Chunk16* t = reinterpret_cast<Chunk16*>(img + trailers[wave - n_entries]);
    t[lane] = Chunk16{{0, 0, 0, 0}};
    return;
  }
  const ZhTarHdrDesc d = descs[wave];
  Chunk16 c{{0, 0, 0, 0}};
  uint32_t sum = 0;
  if (lane < 32) {
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
      const uint32_t v = header_byte(d, pool, lane * 16 + k);
      sum += v;
      c.w[k >> 2] |= v << (8 * (k & 3));
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
  if (lane < 32) {
    if (lane == 9) {  // bytes 148-154 = toOct(sum, 6) & '\0'; 155 stays ' '
      uint32_t o[8];
#pragma unroll
      for (int k = 0; k < 6; k++) o[k] = '0' + ((sum >> (3 * (5 - k))) & 7);
      o[6] = 0;
      o[7] = ' ';
      c.w[1] = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
      c.w[2] = o[4] | (o[5] << 8) | (o[6] << 16) | (o[7] << 24);
    }
    reinterpret_cast<Chunk16*>(img + d.hdr)[lane] = c;
    return;
  }
  // the padding behind the contents (:257-259): chunks [end & ~15, next) of the image
  const uint64_t end = d.hdr + 512 + d.len, next = d.hdr + 512 + ((d.len + 511) & ~(uint64_t)511);
  const uint64_t at = (end & ~(uint64_t)15) + (uint64_t)(lane - 32) * 16;
  if (at >= next) return;
  Chunk16* p = reinterpret_cast<Chunk16*>(img + at);
  Chunk16 z{{0, 0, 0, 0}};
  if (at < end) {  // the straddling chunk: keep its first end - at bytes
    const uint32_t keep = (uint32_t)(end - at);
    z = *p;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint32_t lo = 4 * k;
      z.w[k] = keep >= lo + 4 ? z.w[k] : keep <= lo ? 0u : z.w[k] & ((1u << (8 * (keep - lo))) - 1u);
    }
  }
  *p = z;
}

extern "C" int zh_tar_create_batch(zh_ctx* ctx, const zh_tar_new_entry* entries, const size_t* first, size_t n_tar,
                                   int data_format, int level, void** dsts, size_t* dst_lens, int32_t* statuses) {
  const int bad_call = data_format != ZH_TAR_PLAIN && data_format != ZH_DF_GZIP ? ZH_ERR_INVALID_FORMAT
                       : data_format == ZH_DF_GZIP && (level < -2 || level > 9) ? ZH_ERR_INVALID_LEVEL
                                                                                  : ZH_OK;
  if (const int st = writer_checks(ctx, entries, first, n_tar, bad_call, dsts, dst_lens, statuses); st || !n_tar)
    return st;

  // ---- checks and layout: tarball t's image is [img_off, + img_len) of one buffer, entries back to back ----
  std::vector<ZhTarHdrDesc> descs;
  std::vector<uint64_t> trailers, img_off, img_len, data_off, data_len;
  std::vector<const void*> data_src;
  std::vector<uint8_t> pool;
  std::vector<size_t> ok;  // the tarballs that are written, in order
  uint64_t o = 0;
  for (size_t t = 0; t < n_tar; t++) {
    if (first[t + 1] == first[t]) {  // tarballs_v1.nim:210-211
      statuses[t] = ZH_ERR_TAR_EMPTY;
      continue;
    }
    std::unordered_set<std::string> seen;
    int st = ZH_OK;
    for (size_t i = first[t]; i < first[t + 1] && st == ZH_OK; i++) {
      const zh_tar_new_entry& e = entries[i];
      size_t s = e.path_len;  // std/os splitPath (POSIX): the last '/'
      while (s > 0 && e.path[s - 1] != '/') s--;
      const size_t head = s ? std::max<size_t>(s - 1, 1) : 0, tail = e.path_len - s;
      if (head >= 155)
        st = ZH_ERR_TAR_PATH;  // :218-222
      else if (tail >= 100)
        st = ZH_ERR_TAR_NAME;  // :223-227
      else if ((e.kind != '0' && e.kind != '5') || e.len >= kOct11 || e.mtime < 0 || (uint64_t)e.mtime >= kOct11 ||
               !seen.insert(std::string(e.path ? e.path : "", e.path_len)).second)
        st = ZH_ERR_ARGUMENT;
    }
    if (st != ZH_OK) {
      statuses[t] = st;
      continue;
    }
    ok.push_back(t);
    img_off.push_back(o);
    for (size_t i = first[t]; i < first[t + 1]; i++) {
      const zh_tar_new_entry& e = entries[i];
      size_t s = e.path_len;
      while (s > 0 && e.path[s - 1] != '/') s--;
      ZhTarHdrDesc d{};
      d.hdr = o;
      d.len = e.len;
      d.mtime = (uint64_t)e.mtime;
      d.path = pool.size();
      d.tail_at = (uint32_t)s;
      d.head_len = (uint16_t)(s ? std::max<size_t>(s - 1, 1) : 0);
      d.tail_len = (uint16_t)(e.path_len - s);
      d.kind = (uint8_t)e.kind;
      if (e.path_len) pool.insert(pool.end(), (const uint8_t*)e.path, (const uint8_t*)e.path + e.path_len);
      descs.push_back(d);
      data_off.push_back(o + 512);
      data_len.push_back(e.len);
      data_src.push_back(e.contents);
      o += 512 + ((e.len + 511) & ~(uint64_t)511);
    }
    trailers.push_back(o);
    o += 1024;
    img_len.push_back(o - img_off.back());  // a multiple of 512: the next image starts aligned
  }
  const size_t n_ok = ok.size();
  if (!n_ok) return ZH_OK;
  ZH_HIP(ctx, hipSetDevice(ctx->device));
  Trace tr;

  // ---- descriptors, trailer offsets and names in one upload; the contents straight to their places ----
  DevBuf d_meta, d_img;
  std::vector<uint64_t> moff;
  int st = zhh_upload_spans(ctx,
                            {{descs.data(), descs.size() * sizeof(ZhTarHdrDesc)},
                             {trailers.data(), trailers.size() * 8},
                             {pool.data(), pool.size()}},
                            d_meta, moff);
  if (st) return st;
  if (dev_alloc(ctx, d_img, o + 256) != hipSuccess) return ZH_ERR_NOMEM;
  if ((st = zhh_upload_slices(ctx, data_src.data(), data_off, data_len, o, d_img.p))) return st;
  tr.mark(ctx, "tar: upload");

  const uint64_t waves = descs.size() + trailers.size();
  uint8_t* const img = d_img.p;  // (plain pointers into the launch: a DevBuf is not to be copied)
  const uint8_t* const m = d_meta.p;
  hipLaunchKernelGGL(zh_tar_header_kernel, dim3((uint32_t)((waves + 3) / 4)), dim3(256), 0, ctx->stream, img,
                     reinterpret_cast<const ZhTarHdrDesc*>(m + moff[0]), (uint64_t)descs.size(),
                     reinterpret_cast<const uint64_t*>(m + moff[1]), (uint64_t)trailers.size(), m + moff[2]);
  ZH_HIP(ctx, hipGetLastError());
  tr.mark(ctx, "tar: headers");

  if (data_format == ZH_TAR_PLAIN) {
    st = writer_hand_out(ctx, d_img.p, ok, img_off, img_len, std::vector<int32_t>(n_ok, ZH_OK), dsts, dst_lens,
                         statuses);
  } else {  // compress(data, level, dfGzip) of every image, one plan
    DevBuf d_dst;
    std::vector<uint64_t> doff, clen;
    std::vector<int32_t> cst;
    if ((st = zhh_compress(ctx, d_img.p, img_off, img_len, level, ZH_DF_GZIP, nullptr, d_dst, doff, clen, cst)))
      return st;
    tr.mark(ctx, "tar: compress");
    st = writer_hand_out(ctx, d_dst.p, ok, doff, clen, cst, dsts, dst_lens, statuses);
  }
  if (st) return st;
  tr.mark(ctx, "tar: download");
  return ZH_OK;
}
