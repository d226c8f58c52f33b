// Batched inflate: container unwrap + RFC 1951 decode, one workgroup of two 64-lane waves
// per stream (a foreign deflate stream has no block index, so the only parallelism across a
// stream is lane-level; throughput comes from thousands of streams -- or, for streams this
// library wrote with a block index, from zh_plan_uncompress_indexed, which makes every block
// a "stream" of this kernel).
//
// Replaces src/zippy.nim:100-165 (format detect / zlib header), gzip.nim:3-88
// (gzip header + trailer), inflate.nim:24-291 (Huffman tables, decode loop,
// stored blocks) and the BitStreamReader of bitstreams.nim:22-82.
//
// Per workgroup, in LDS (9.3 KiB, 16 workgroups = 32 waves per CU -- a wave alone on its SIMD
// issues one instruction per ~4.4 cycles, so resident waves are what buys throughput): a 10-bit
// literal/length root LUT with second-level tables behind it for longer codes and an 8-bit
// distance LUT, all of self-describing 32-bit entries (inflate.nim's 9-bit `fast` table,
// re-shaped), the canonical slow-path arrays (firstCode / firstSymbol / maxCodes / values,
// inflate.nim:14-19), a 512-byte staging ring of the compressed stream and two round
// descriptors.  There is no window copy: the LZ window is the output itself, read back through
// L2.  The decode wave and the output wave are described in zh_inflate_pair.h, which holds the kernel's body.
// Algorithmic traffic: compressed bytes read once, output written once.
#include "zh_common.h"
#include "zh_kprof.h"
#include "zh_tables.h"
#include "zh_inflate_header.h"
#include "zh_inflate_pair.h"


// ---------------------------------------------------------------------------
// Container unwrap: one thread per stream.
// ---------------------------------------------------------------------------
__global__ void zh_unwrap_kernel(const uint8_t* __restrict__ d_src, ZhInflateArgs a) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.nbufs) return;
  const ZhBufDesc b = a.bufs[i];
  const uint8_t* src = d_src + b.src_off;
  const uint64_t len = a.src_len_dev ? a.src_len_dev[i] : b.src_len;
  int fmt = a.data_format;
  int st = ZH_OK;
  uint32_t pos = 0, sum = 0, isize = 0;

  if (fmt == ZH_DF_DETECT) {  // zippy.nim:108-125
    if (len > 18 && src[0] == 31 && src[1] == 139 && src[2] == 8 && (src[3] & 0xe0) == 0)
      fmt = ZH_DF_GZIP;
    else if (len > 6 && (src[0] & 0x0f) == 8 && (src[0] >> 4) <= 7 &&
             (((uint32_t)src[0] * 256u) + src[1]) % 31u == 0)
      fmt = ZH_DF_ZLIB;
    else
      st = ZH_ERR_DETECT;
  }
  if (st == ZH_OK && fmt == ZH_DF_GZIP) {  // gzip.nim:9-66
    if (len < 18) {
      st = ZH_ERR_INVALID_BUFFER;
    } else {
      const uint8_t flg = src[3];
      if (src[0] != 31 || src[1] != 139) st = ZH_ERR_GZIP_ID;
      else if (src[2] != 8) st = ZH_ERR_UNSUPPORTED_METHOD;
      else if (flg & 0xe0) st = ZH_ERR_RESERVED_FLAGS;
      else if (flg & 4) st = ZH_ERR_UNSUPPORTED_FLAGS;  // FEXTRA
      uint64_t p = 10;
      for (int field = 0; field < 2 && st == ZH_OK; field++) {  // FNAME, FCOMMENT
        if (flg & (field == 0 ? 8 : 16)) {
          while (p < len && src[p] != 0) p++;
          if (p >= len) st = ZH_ERR_INVALID_BUFFER;
          p++;
        }
      }
      if (st == ZH_OK && (flg & 2)) {  // FHCRC: skipped, not verified (gzip.nim:55-59)
        if (p + 2 >= len) st = ZH_ERR_INVALID_BUFFER;
        p += 2;
      }
      if (st == ZH_OK && p + 8 >= len) st = ZH_ERR_INVALID_BUFFER;
      if (st == ZH_OK) {
        pos = (uint32_t)p;
        const uint8_t* t = src + len - 8;
        sum = t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24);
        isize = t[4] | (t[5] << 8) | (t[6] << 16) | ((uint32_t)t[7] << 24);
      }
    }
  } else if (st == ZH_OK && fmt == ZH_DF_ZLIB) {  // zippy.nim:130-150
    if (len < 6) {
      st = ZH_ERR_INVALID_BUFFER;
    } else {
      const uint8_t cmf = src[0], flg = src[1];
      if ((cmf & 0x0f) != 8) st = ZH_ERR_UNSUPPORTED_METHOD;
      else if ((cmf >> 4) > 7) st = ZH_ERR_COMPRESSION_INFO;
      else if ((((uint32_t)cmf * 256u) + flg) % 31u != 0) st = ZH_ERR_INVALID_HEADER;
      else if (flg & 0x20) st = ZH_ERR_PRESET_DICT;
      pos = 2;
      const uint8_t* t = src + len - 4;
      sum = ((uint32_t)t[0] << 24) | (t[1] << 16) | (t[2] << 8) | t[3];
    }
  } else if (st == ZH_OK && fmt != ZH_DF_DEFLATE) {
    st = ZH_ERR_INVALID_FORMAT;
  }
  a.body_pos[i] = pos;
  a.fmt[i] = (uint32_t)fmt;
  a.expect_sum[i] = sum;
  a.expect_isize[i] = isize;
  a.status[i] = st;
  a.out_len[i] = 0;
}


__global__ __launch_bounds__(128, 8) void zh_inflate_kernel(const uint8_t* __restrict__ d_src,
                                                         uint8_t* __restrict__ d_dst,
                                                         ZhInflateArgs a) {
  zh_inflate_body<kFormBatch>(d_src, d_dst, a, ZhSeekStop{}, ZhResume{});
}

// Final check of each stream against its trailer (gzip.nim:80-88, zippy.nim:152-162).
__global__ void zh_verify_kernel(ZhInflateArgs a, const uint32_t* __restrict__ buf_crc,
                                 const uint32_t* __restrict__ buf_adler) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.nbufs) return;
  if (a.status[i] != ZH_OK) return;
  const uint32_t fmt = a.fmt[i];
  if (fmt == ZH_DF_GZIP) {
    if (a.expect_sum[i] != buf_crc[i]) a.status[i] = ZH_ERR_CHECKSUM;
    else if (a.expect_isize[i] != (uint32_t)(a.out_len[i] & 0xffffffffu)) a.status[i] = ZH_ERR_SIZE;
  } else if (fmt == ZH_DF_ZLIB) {
    if (a.expect_sum[i] != buf_adler[i]) a.status[i] = ZH_ERR_CHECKSUM;
  }
}

// Block-parallel decode: fold the per-block results into the stream's.  Every block must have
// produced exactly the bytes its index entry promised.
__global__ __launch_bounds__(64) void zh_segments_reduce_kernel(ZhInflateArgs seg, ZhInflateArgs stream) {
  __shared__ uint64_t s_total[64];
  __shared__ uint32_t s_bad[64];
  const unsigned lane = zh_lane();
  uint64_t total = 0;
  uint32_t bad = 0xffffffffu;
  for (uint32_t i = lane; i < seg.nbufs; i += 64) {
    const uint64_t len = seg.out_len[i];
    total += len;
    if ((seg.status[i] != ZH_OK || len != seg.bufs[i].dst_cap) && i < bad) bad = i;
  }
  s_total[lane] = total;
  s_bad[lane] = bad;
  zh_wave_sync();
  if (lane == 0 && stream.status[0] == ZH_OK) {
    for (uint32_t l = 1; l < 64; l++) {
      total += s_total[l];
      if (s_bad[l] < bad) bad = s_bad[l];
    }
    stream.out_len[0] = total;
    if (bad != 0xffffffffu) {
      const int32_t st = seg.status[bad];
      stream.status[0] = (st == ZH_OK || st == ZH_ERR_DST_TOO_SMALL) ? (int32_t)ZH_ERR_INVALID_BUFFER : st;
    }
  }
}

extern "C" void zh_launch_segments_reduce(hipStream_t stream, ZhInflateArgs seg, ZhInflateArgs whole) {
  hipLaunchKernelGGL(zh_segments_reduce_kernel, dim3(1), dim3(64), 0, stream, seg, whole);
}

extern "C" void zh_launch_unwrap(hipStream_t stream, const uint8_t* d_src, ZhInflateArgs a) {
  if (!a.nbufs) return;
  hipLaunchKernelGGL(zh_unwrap_kernel, dim3((a.nbufs + 63) / 64), dim3(64), 0, stream, d_src, a);
}
extern "C" void zh_launch_inflate(hipStream_t stream, const uint8_t* d_src, uint8_t* d_dst,
                                  ZhInflateArgs a) {
  if (!a.nbufs) return;
  hipLaunchKernelGGL(zh_inflate_kernel, dim3(a.nbufs), dim3(128), 0, stream, d_src, d_dst, a);
}
extern "C" void zh_launch_verify(hipStream_t stream, ZhInflateArgs a, const uint32_t* buf_crc,
                                 const uint32_t* buf_adler) {
  if (!a.nbufs) return;
  hipLaunchKernelGGL(zh_verify_kernel, dim3((a.nbufs + 63) / 64), dim3(64), 0, stream, a, buf_crc,
                     buf_adler);
}
