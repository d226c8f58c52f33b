/*
 * zippy_hip.h -- C ABI of the MI355X-native batched DEFLATE engine.
 *
 * This is the drop-in boundary for guzba/zippy's compress()/uncompress() path.
 * zippy has no FFI/plugin interface of its own: the boundary is its exported
 * Nim procs, so every entry point below cites the Nim proc it stands behind
 * (file:line under the reference tree).  A Nim shim that binds these symbols
 * and re-exposes zippy's exact signatures is in INTEGRATION.md.
 *
 * Plain C: pointers, sizes, status codes.  No torch types, no C++ types.
 * All work runs on one GPU through hand-written gfx950 kernels; there is no
 * CPU fallback (calls fail with ZH_ERR_DEVICE if no GPU is usable).
 */
#ifndef ZIPPY_HIP_H
#define ZIPPY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* CompressedDataFormat, src/zippy/common.nim:4-5 (same ordinals) */
enum { ZH_DF_DETECT = 0, ZH_DF_ZLIB = 1, ZH_DF_GZIP = 2, ZH_DF_DEFLATE = 3 };

/* Levels, src/zippy/common.nim:7-12; valid range -2..9 (deflate.nim:208-209) */
enum {
  ZH_NO_COMPRESSION = 0,
  ZH_BEST_SPEED = 1,
  ZH_BEST_COMPRESSION = 9,
  ZH_DEFAULT_COMPRESSION = -1,
  ZH_HUFFMAN_ONLY = -2
};

/* Status codes.  1..18 map one-to-one onto the ZippyError raise sites of the
 * reference; zh_strerror() returns the reference's message. */
enum {
  ZH_OK = 0,
  ZH_ERR_INVALID_LEVEL = 1,      /* deflate.nim:208-209 */
  ZH_ERR_INVALID_FORMAT = 2,     /* zippy.nim:83-84 */
  ZH_ERR_DETECT = 3,             /* zippy.nim:125 */
  ZH_ERR_UNSUPPORTED_METHOD = 4, /* zippy.nim:141, gzip.nim:26 */
  ZH_ERR_COMPRESSION_INFO = 5,   /* zippy.nim:144 */
  ZH_ERR_INVALID_HEADER = 6,     /* zippy.nim:147 */
  ZH_ERR_PRESET_DICT = 7,        /* zippy.nim:150 */
  ZH_ERR_CHECKSUM = 8,           /* zippy.nim:162, gzip.nim:81 */
  ZH_ERR_SIZE = 9,               /* gzip.nim:85,88 */
  ZH_ERR_GZIP_ID = 10,           /* gzip.nim:23 */
  ZH_ERR_RESERVED_FLAGS = 11,    /* gzip.nim:29 */
  ZH_ERR_UNSUPPORTED_FLAGS = 12, /* gzip.nim:41 */
  ZH_ERR_INVALID_BUFFER = 13,    /* internal.nim:191-192 */
  ZH_ERR_COMPRESS_INTERNAL = 14, /* internal.nim:194-195 */
  ZH_ERR_END_OF_BUFFER = 15,     /* bitstreams.nim:16-17 */
  ZH_ERR_BYTE_BOUNDARY = 16,     /* bitstreams.nim:66,113 */
  ZH_ERR_BLOCK_HEADER = 17,      /* inflate.nim:289 */
  ZH_ERR_INVALID_SYMBOL = 18,    /* inflate.nim:165 */
  ZH_ERR_NOMEM = 19,             /* host or device allocation failed */
  ZH_ERR_DEVICE = 20,            /* no usable GPU / HIP runtime error (zh_last_error) */
  ZH_ERR_DST_TOO_SMALL = 21,     /* device API: output slot capacity exceeded */
  ZH_ERR_ARGUMENT = 22,          /* NULL pointer, bad plan, ... */
  /* archive layer (zh_zip_*): the ZippyError raise sites of ziparchives.nim */
  ZH_ERR_ARCHIVE_EOF = 23,        /* internal.nim:197-198 failArchiveEOF */
  ZH_ERR_ZIP_FILE_HEADER = 24,    /* ziparchives.nim:58-59 */
  ZH_ERR_ZIP_METHOD = 25,         /* ziparchives.nim:87-88,296-297 */
  ZH_ERR_ZIP_NO_RECORD = 26,      /* ziparchives.nim:43-52,89-90 */
  ZH_ERR_ZIP_CRC = 27,            /* ziparchives.nim:91-92 */
  ZH_ERR_ZIP_UNSUPPORTED = 28,    /* ziparchives.nim:214-218,248-255 disk / record numbers */
  ZH_ERR_ZIP_CENTRAL_HEADER = 29, /* ziparchives.nim:224-225,279-280 */
  ZH_ERR_ZIP_DISK_NUMBER = 30,    /* ziparchives.nim:299-300 */
  ZH_ERR_ZIP_DUPLICATE = 31,      /* ziparchives.nim:314-315 */
  ZH_ERR_ZIP_CENTRAL_SIZE = 32,   /* ziparchives.nim:343-344 */
  ZH_ERR_ZIP_NAME = 33,           /* ziparchives.nim:506-511 empty / absolute / over-long path */
  ZH_ERR_TAR_HEADER_TYPE = 34,    /* tarballs.nim:119 */
  ZH_ERR_UNSAFE_PATH = 35,        /* internal.nim:294-302 verifyPathIsSafeToExtract */
  ZH_ERR_TAR_NUMBER = 36,         /* tarballs.nim:17-23 (octal field that is not octal) */
  /* tarball writer (zh_tar_create_batch): the ZippyError raise sites of tarballs_v1.nim writeTarball */
  ZH_ERR_TAR_EMPTY = 37,          /* tarballs_v1.nim:210-211 */
  ZH_ERR_TAR_PATH = 38,           /* tarballs_v1.nim:218-222 (splitPath head >= 155 bytes) */
  ZH_ERR_TAR_NAME = 39,           /* tarballs_v1.nim:223-227 (splitPath tail >= 100 bytes) */
  /* v1 zip writer (zh_zip_write_batch): ziparchives_v1.nim writeZipArchive */
  ZH_ERR_ZIP_EMPTY = 40,          /* ziparchives_v1.nim:375-376 */
  ZH_ERR_ZIP_TOO_LARGE = 41,      /* a count, length or offset that does not fit its 16- / 32-bit field */
  /* v1 zip reader (zh_zip_read_batch): ziparchives_v1.nim openStreamImpl */
  ZH_ERR_ZIP_DATA_DESCRIPTOR = 42, /* ziparchives_v1.nim:138-142 */
  ZH_ERR_ZIP_DEFLATE64 = 43,       /* ziparchives_v1.nim:144-148 (flag bit 3) */
  ZH_ERR_ZIP_SIZE = 44,            /* ziparchives_v1.nim:213-217 */
  ZH_ERR_ZIP_OPEN = 45,            /* ziparchives_v1.nim:110-111 failOpen: :282-293, :328-329 */
  /* v1 tarball reader (zh_tar_read_batch): tarballs_v1.nim openStreamImpl */
  ZH_ERR_TAR_FORMAT = 46,          /* tarballs_v1.nim:86 */
  ZH_ERR_TAR_OPEN = 47,            /* tarballs_v1.nim:118,124 (size or mtime that parseOctInt rejects) */
  ZH_ERR_TAR_OPEN_MODE = 48,       /* tarballs_v1.nim:131 */
  ZH_ERR_TAR_EOF = 49,             /* tarballs_v1.nim:61-64 failEOF */
  /* BGZF (zh_bgzf_*): SAM specification, section 4.1 */
  ZH_ERR_BGZF_HEADER = 50          /* extra field without a BC subfield, subfields that do not tile XLEN, BSIZE too
                                      small for the member's own header + trailer, ISIZE > 65536 */
};

/* Engine context: one GPU, one HIP stream, reusable scratch. Thread-compatible
 * (one thread at a time per context; separate contexts are independent), like
 * the reference's re-entrant pure procs (SURVEY.md 8b "Threading"). */
typedef struct zh_ctx zh_ctx;

/* device < 0: current device.  stream: a hipStream_t to enqueue on, or NULL to
 * let the context create its own. */
int zh_create(int device, void *stream, zh_ctx **out);
/* The chain levels' (-1, 2..9) link kernels take the ORDER of their results from a property of the LDS
 * unit -- the lanes of one returning atomic are served in ascending lane order -- which the ISA manual does
 * not promise (lz77.nim:69-71's `chain[windowPos] = head[hash]; head[hash] = windowPos`, 64 positions a
 * step).  zh_create asks the device itself, once per device and process (a known-answer launch on the
 * context's stream, which it waits for); a device that answers otherwise gets the in-order link kernels
 * -- same bytes, slower -- and zh_last_error says so.  -> 1: the device passed, 0: the in-order kernels run
 * (also under ZH_CHAIN_PREV=serial). */
int zh_chain_links_parallel(zh_ctx *ctx);
void zh_destroy(zh_ctx *ctx);
const char *zh_strerror(int status);
const char *zh_last_error(zh_ctx *ctx); /* detail of the last ZH_ERR_DEVICE */
void *zh_stream(zh_ctx *ctx);           /* the hipStream_t work is enqueued on */

/* gzip FNAME length: the reference inserts 0..25 letters chosen at random per
 * call (zippy.nim:26-42).  k < 0 (default): random per buffer like the
 * reference; 0..25: fixed (deterministic output for tests). */
void zh_set_gzip_fname_len(zh_ctx *ctx, int k);

/* Which inflate kernels later uncompress calls of this context use (no reference counterpart;
 * same results either way): 0 = a stream's Huffman codes decoded in parallel, then one writer
 * per stream (csrc/zh_inflate_split.hip); 1 = the two-wave serial decoder (csrc/zh_inflate.hip);
 * < 0 = the default (0, or the ZH_INFLATE=serial environment variable). */
void zh_set_inflate_mode(zh_ctx *ctx, int mode);

/* Which BestSpeed (level 1) match finder later compress calls of this context use.
 * 0 = the reference's parse (snappy.nim:12-136 replayed decision for decision: the streams are
 * byte-identical to zippy's own); 1 = the parallel parse of csrc/zh_l1p_match.hip: every position
 * enters the hash table and the greedy selection runs chunk-parallel, so the token stream differs
 * from zippy's while meeting the encoder contract -- a valid RFC 1951/1950/1952 stream that zippy's
 * uncompress() decodes to the input bit for bit, compressed size within 2 % of zippy's at level 1
 * (tests/test_gpu_parity.py: test_gpu_parallel_parse_*); its tokens are those of the serial rule
 * of tests/l1p_model.py, token for token (test_gpu_l1p_tokens, test_gpu_l1p_streams,
 * test_gpu_l1p_alignment: crafted family P of tests/parity_cases.py).  < 0 = the default (0, or the
 * ZH_L1_PARSE=parallel environment variable).  All other levels are unaffected. */
void zh_set_l1_parse(zh_ctx *ctx, int mode);

/* Host-buffer compress calls of at least min_batch_bytes of input run as pipelined groups of
 * about group_bytes each: one group's kernels overlap the neighbours' transfers (no reference
 * counterpart; the results are the same bytes either way).  0 = default (1 GiB / 512 MiB, or the
 * ZH_PIPE_MIN / ZH_PIPE_GROUP environment variables). */
void zh_set_host_pipeline(zh_ctx *ctx, size_t min_batch_bytes, size_t group_bytes);

/* Upper bound of compress() output for len input bytes: stored form
 * len + 5*ceil(len/65535) (deflate.nim:179-205) + container + slack. */
size_t zh_compress_bound(size_t len, int data_format);

/* ------------------------------------------------------------------ *
 * Host-buffer API: what the Nim shim binds.                           *
 * Inputs are borrowed read-only for the call; outputs are freshly     *
 * allocated by the library (release with zh_free) -- the ownership    *
 * model of `compress*(...): string` (zippy.nim:11-16).               *
 * ------------------------------------------------------------------ */

/* compress*(src: pointer, len, level, dataFormat): string -- zippy.nim:11-84,
 * for n independent buffers at once.  statuses[i] is per buffer; the return
 * value is ZH_OK unless the call as a whole could not run. */
int zh_compress_batch(zh_ctx *ctx, const void *const *srcs, const size_t *lens, size_t n,
                      int level, int data_format, void **dsts, size_t *dst_lens,
                      int32_t *statuses);

/* uncompress*(src: pointer, len, dataFormat): string -- zippy.nim:100-165,
 * gzip.nim:3-88, for n independent streams at once.  A bad stream only fails
 * its own slot. */
int zh_uncompress_batch(zh_ctx *ctx, const void *const *srcs, const size_t *lens, size_t n,
                        int data_format, void **dsts, size_t *dst_lens, int32_t *statuses);

/* The two calls above with the results in buffers of the CALLER'S: dsts[i] (caps[i] bytes) on
 * entry.  No reference counterpart -- zippy returns fresh strings (zippy.nim:11-18,100-104) -- but
 * what a binding that owns its strings wants: the shim allocates `newString(zh_compress_bound(n))`
 * (or a string of ISIZE bytes), the library fills it, and the only copy left is the one from the
 * pinned staging chunk.  A result that does not fit: statuses[i] = ZH_ERR_DST_TOO_SMALL and
 * dst_lens[i] = the size it needs.  On return dsts[i] is the caller's pointer for every buffer that
 * was filled and NULL otherwise; nothing here goes to zh_free.  For streams without a size field
 * (zlib, raw deflate) caps[i] is also how much is decoded at most before the expansion bound is
 * tried. */
int zh_compress_batch_into(zh_ctx *ctx, const void *const *srcs, const size_t *lens, size_t n,
                           int level, int data_format, void **dsts, const size_t *caps,
                           size_t *dst_lens, int32_t *statuses);
int zh_uncompress_batch_into(zh_ctx *ctx, const void *const *srcs, const size_t *lens, size_t n,
                             int data_format, void **dsts, const size_t *caps, size_t *dst_lens,
                             int32_t *statuses);

/* One batch over several GPUs of a node.  zippy's compress()/uncompress() are pure functions of
 * one buffer (zippy.nim:11-16,100-104), so a batch shards by contiguous index ranges with no
 * exchange step: context r (one per device, made with zh_create(r, NULL, &ctx[r])) takes range r
 * of the batch -- the first n % n_ctx ranges hold one buffer more -- on its own host thread, and
 * every result lands in the caller's arrays at its own index.  Same results as the
 * single-context calls.  Contexts must be distinct; two contexts on ONE device are allowed
 * (they share the GPU).  Returns the first failing shard's call status, else ZH_OK. */
int zh_device_count(void);
int zh_compress_batch_multi(zh_ctx *const *ctxs, size_t n_ctx, const void *const *srcs,
                            const size_t *lens, size_t n, int level, int data_format, void **dsts,
                            size_t *dst_lens, int32_t *statuses);
int zh_uncompress_batch_multi(zh_ctx *const *ctxs, size_t n_ctx, const void *const *srcs,
                              const size_t *lens, size_t n, int data_format, void **dsts,
                              size_t *dst_lens, int32_t *statuses);

/* Single-buffer forms (batch of 1); return the buffer's status. */
int zh_compress(zh_ctx *ctx, const void *src, size_t len, int level, int data_format,
                void **dst, size_t *dst_len);
int zh_uncompress(zh_ctx *ctx, const void *src, size_t len, int data_format, void **dst,
                  size_t *dst_len);

/* crc32*(src: pointer, len): uint32 -- crc.nim:53-72 ; adler32* -- adler32.nim:6 */
int zh_crc32(zh_ctx *ctx, const void *src, size_t len, uint32_t *out);
int zh_adler32(zh_ctx *ctx, const void *src, size_t len, uint32_t *out);

/* n checksums in one launch pair: crc32* applied to every buffer (crc.nim:53-72). */
int zh_crc32_batch(zh_ctx *ctx, const void *const *srcs, const size_t *lens, size_t n, uint32_t *out);

/* zh_compress_batch that also returns crc32(srcs[i]) -- what createZipArchive needs per entry
 * (ziparchives.nim:526-530: crc32(contents); compress(contents, BestSpeed, dfDeflate)). */
int zh_compress_batch_crc32(zh_ctx *ctx, const void *const *srcs, const size_t *lens, size_t n,
                            int level, int data_format, void **dsts, size_t *dst_lens,
                            int32_t *statuses, uint32_t *crcs);
/* zh_uncompress_batch for callers that know the output sizes up front (ZIP central directory,
 * ziparchives.nim:85-93; gzip.nim:72-76 trustSize): size_hints[i] replaces the guess (4x the
 * stream, then a sizing pass if that was too little) of zlib/raw streams (a wrong hint only costs a retry), crcs[i] (optional) = crc32 of output i. */
int zh_uncompress_batch_sized(zh_ctx *ctx, const void *const *srcs, const size_t *lens, size_t n,
                              int data_format, const uint64_t *size_hints, void **dsts,
                              size_t *dst_lens, int32_t *statuses, uint32_t *crcs);

void zh_free(void *p);

/* ------------------------------------------------------------------ *
 * Device-resident API: buffers already in HBM (pipelines, bench.py).  *
 * A plan owns the device-side descriptors and scratch for one batch   *
 * geometry; running it only enqueues kernels on the context's stream  *
 * (no host synchronisation), so it can be timed with HIP events or    *
 * captured in a hipGraph.                                             *
 * ------------------------------------------------------------------ */
typedef struct zh_plan zh_plan;

/* Device memory for a caller without a HIP binding of its own (a Nim / cgo / JNI shim that drives the plans; callers
 * that have one -- hipMalloc, a torch tensor's data_ptr -- pass their own pointers): blocks of the context's device,
 * copies on the context's stream and waited for.  zh_device_free waits for the stream first. */
int zh_device_malloc(zh_ctx *ctx, size_t bytes, void **d_out);
void zh_device_free(zh_ctx *ctx, void *d);
int zh_device_upload(zh_ctx *ctx, void *d_dst, const void *src, size_t bytes);
int zh_device_download(zh_ctx *ctx, void *dst, const void *d_src, size_t bytes);

/* Buffer i is d_src[src_off[i] .. +src_len[i]); its output slot is
 * d_dst[dst_off[i] .. +dst_cap[i]).  Offsets are in bytes. */
int zh_plan_compress(zh_ctx *ctx, size_t n, const uint64_t *src_off, const uint64_t *src_len,
                     const uint64_t *dst_off, const uint64_t *dst_cap, int level,
                     int data_format, zh_plan **out);
/* An uncompress plan of a handful of streams (its longest stream weighs more than 1/40 of the batch
 * + 8 MiB) decodes every stream of >= 128 KiB with many workgroups (block starts searched for,
 * decoded from at once, proved afterwards; same bytes and statuses as one decoder per stream, which
 * remains the fallback stream by stream).  Its scratch -- about 45 bytes per compressed byte --
 * is allocated at the plan's first run; ZH_SEG=0 in the environment turns this off. */
int zh_plan_uncompress(zh_ctx *ctx, size_t n, const uint64_t *src_off, const uint64_t *src_len,
                       const uint64_t *dst_off, const uint64_t *dst_cap, int data_format,
                       zh_plan **out);
/* Enqueue the plan. d_src/d_dst are device pointers.
 * Preconditions and side effects (compress plans):
 *  - d_dst must be 4-byte aligned (the encoder addresses the output as 32-bit words; slot
 *    offsets themselves may be any byte); a misaligned d_dst returns ZH_ERR_ARGUMENT;
 *  - nothing is cleared beforehand and nothing but a stream's own bytes is written: of slot i only
 *    [dst_off, dst_off + out_len) changes -- whatever the slot held before --, the rest of the slot and
 *    the bytes of d_dst between slots keep their contents (until round 6 the whole slot was zeroed first);
 *  - slots must not overlap.
 * Both directions read whole aligned 32-bit words around a source buffer, i.e. up to 3 bytes
 * before src_off and after src_off + src_len: those bytes must be mapped (true inside any
 * hipMalloc allocation, which is 256-byte aligned and padded); their values are ignored.
 * Uncompress plans: on ZH_ERR_DST_TOO_SMALL out_len is the number of leading bytes of the slot
 * that hold valid output (out_len <= dst_cap; 0 for a large stream decoded segment-wise, which
 * writes nothing once it knows the slot is too small), not the required size; callers that need
 * the size use the host-buffer calls (which size and retry) or a larger slot. */
int zh_plan_run(zh_plan *plan, const void *d_src, void *d_dst);
/* Wait for the stream and fetch per-buffer output lengths and statuses. */
int zh_plan_results(zh_plan *plan, uint64_t *out_lens, int32_t *statuses);
/* Device arrays of the same (uint64 lens[n], int32 statuses[n]); valid after run. */
const uint64_t *zh_plan_device_lens(zh_plan *plan);
const int32_t *zh_plan_device_statuses(zh_plan *plan);
/* Re-point an uncompress plan at new per-stream compressed lengths (same
 * offsets/capacities), e.g. after a compress plan produced them on device. */
int zh_plan_set_src_lens_device(zh_plan *plan, const uint64_t *d_lens);
/* Whole buffers on their way between GPUs (zippy.nim:11-18: a buffer is compressed / uncompressed by itself, so a
 * batch is sharded by handing whole buffers around and nothing else ever travels).  Output slots have the worst-case
 * size; what goes over a link is the streams alone:
 *  - zh_plan_pack, after zh_plan_run: result i of the plan (d_slots + dst_off[i], zh_plan_device_lens()[i] bytes; 0
 *    bytes where the status is not ZH_OK) is copied to d_packed + d_offsets[i], back to back: d_offsets[0] = 0,
 *    d_offsets[i + 1] = d_offsets[i] + length i -- n + 1 device uint64, written by the call.  Nothing is written at
 *    or beyond d_packed + packed_cap (a caller that sized d_packed too small sees d_offsets[n] > packed_cap).
 *  - zh_plan_unpack, before zh_plan_run of an UNCOMPRESS plan: stream i (d_packed + d_offsets[i], d_offsets[i + 1] -
 *    d_offsets[i] bytes, at most the src_len[i] the plan was made with: the slot's size) is copied to d_slots +
 *    src_off[i], and the plan decodes streams of these lengths from now on (as after zh_plan_set_src_lens_device --
 *    and, like there, for good: the plan's segment geometry was laid over the lengths it was made with, so from the
 *    first unpack on it decodes every stream with one workgroup, large ones included; make a new plan to get the
 *    segment-wise decode of large streams back).  ZH_ERR_ARGUMENT (more than 2^31 copy workgroups) is returned before
 *    anything is launched or written, for both calls.
 * Device pointers throughout, kernel launches on the context's stream only, no host synchronisation: a pack may
 * follow a run, a run an unpack, at once. */
int zh_plan_pack(zh_plan *plan, const void *d_slots, void *d_packed, uint64_t packed_cap, uint64_t *d_offsets);
int zh_plan_unpack(zh_plan *plan, const void *d_packed, const uint64_t *d_offsets, void *d_slots);
void zh_plan_destroy(zh_plan *plan);

/* CRC-32 of the uncompressed side of every buffer (sources of a compress plan, outputs of an
 * uncompress plan) whatever the container: request before zh_plan_run, read after it. */
int zh_plan_request_crc32(zh_plan *plan, int on);
int zh_plan_crc32(zh_plan *plan, uint32_t *crcs);

/* Per-kernel timing of the LAST zh_plan_run when profiling is on (HIP events on
 * the context's stream around every launch).  names[i] are static strings. */
void zh_plan_set_profiling(zh_plan *plan, int on);
int zh_plan_kernel_times(zh_plan *plan, const char **names, float *ms, int max_entries);

/* ------------------------------------------------------------------ *
 * Block-parallel form of ONE large buffer (BASELINE.json config 5).   *
 * The reference cuts a buffer into deflate blocks of 4 MiB            *
 * (deflate.nim:228, internal.nim:16) and calls the matcher once per   *
 * block (deflate.nim:243-272), so no match ever reaches across a      *
 * block start: a block can be decoded by itself once its bit position *
 * is known.  These entry points expose that: the same encoder with    *
 * the block size as a parameter (block_bytes: a multiple of 32768,    *
 * 32768 .. 4194304; 4194304 reproduces zh_compress byte for byte),    *
 * and the index of block starts that lets the decoder run one wave    *
 * pair per block instead of one per stream.  The stream stays plain   *
 * RFC 1951/1950/1952: zippy's uncompress() (and zh_uncompress) decode *
 * it without the index.                                               *
 * ------------------------------------------------------------------ */
typedef struct zh_block_entry {
  uint64_t bit_off; /* block's BFINAL bit, in bits from the start of the compressed buffer */
  uint64_t out_off; /* offset of the block's first byte in the uncompressed data */
} zh_block_entry;

/* index: library-allocated (zh_free), n_entries = deflate blocks + 1; the closing entry holds
 * the bit just past the last block and the uncompressed length.  A stored logical block longer
 * than 65535 bytes contributes one entry per stored chunk (deflate.nim:179-205). */
int zh_compress_blocks(zh_ctx *ctx, const void *src, size_t len, int level, int data_format,
                       size_t block_bytes, void **dst, size_t *dst_len, zh_block_entry **index,
                       size_t *n_entries);
/* Decode with one decoder per index entry.  Fails with ZH_ERR_INVALID_BUFFER when a block does
 * not produce exactly the bytes its entry promises (or reaches back before its own start);
 * container checks and checksum as in zh_uncompress. */
int zh_uncompress_indexed(zh_ctx *ctx, const void *src, size_t len, int data_format,
                          const zh_block_entry *index, size_t n_entries, void **dst,
                          size_t *dst_len);

/* Device-resident forms.  zh_plan_compress_blocks = zh_plan_compress with the block size;
 * after zh_plan_run + zh_plan_results, zh_plan_block_index returns buffer `buf`'s index
 * (library-allocated, zh_free).  zh_plan_uncompress_indexed plans ONE stream
 * d_src[src_off .. +src_len) -> d_dst[dst_off .. +dst_cap) with its index (host array). */
int zh_plan_compress_blocks(zh_ctx *ctx, size_t n, const uint64_t *src_off, const uint64_t *src_len,
                            const uint64_t *dst_off, const uint64_t *dst_cap, int level,
                            int data_format, size_t block_bytes, zh_plan **out);
int zh_plan_block_index(zh_plan *plan, size_t buf, zh_block_entry **index, size_t *n_entries);
int zh_plan_uncompress_indexed(zh_ctx *ctx, uint64_t src_off, uint64_t src_len, uint64_t dst_off,
                               uint64_t dst_cap, int data_format, const zh_block_entry *index,
                               size_t n_entries, zh_plan **out);

/* Byte ranges of the UNCOMPRESSED data of block-indexed streams, many ranges of many streams in one call: only the
 * blocks a range touches are decoded (and, from host buffers, only their compressed bytes uploaded).
 *
 * Device-resident: stream s is d_src[src_off[s] .. +src_len[s]) with index entries
 * index[first[s] .. first[s+1]) (each stream's list closed as zh_compress_blocks returns it).
 * Range r reads bytes [range_off[r], range_off[r]+range_len[r]) of the UNCOMPRESSED data of stream
 * range_stream[r] into d_dst[dst_off[r] .. +dst_cap[r]).
 *
 * Ranges read like pread:
 *  - a range is clipped at the stream's uncompressed length (the closing entry's out_off); range_off at or beyond it,
 *    or range_len 0, gives 0 bytes and ZH_OK and touches no block; range_off + range_len beyond 2^64 is clipped too;
 *  - range_stream[r] >= n_streams and NULL arrays are the caller's bugs: ZH_ERR_ARGUMENT, nothing runs;
 *  - a stream whose index cannot be right -- fewer than 2 entries, out_off or bit_off falling, index[0].out_off != 0,
 *    a block's bit_off at or beyond 8 * src_len, a block that promises more than 1032 * (its compressed bytes) + 64
 *    bytes -- fails every range of THAT stream with ZH_ERR_INVALID_BUFFER; other streams' ranges are not affected.
 * What is verified: neither the container's header nor its trailer is looked at (a range cannot prove a checksum of
 * the whole, and bit_off counts from the first byte of the buffer whatever the container).  Every block a range
 * touches must decode with ZH_OK and make exactly out_off[k+1] - out_off[k] bytes; otherwise the range's status is
 * that of its lowest such block (ZH_OK and ZH_ERR_DST_TOO_SMALL of a block read ZH_ERR_INVALID_BUFFER, as in
 * zh_uncompress_indexed), its length 0 and its slot's contents unspecified.  Ranges that touch no bad block succeed.
 * A match that reaches back before its block's start (a stream not written block-parallel) fails the range the same
 * way.
 * A slot smaller than the clipped range (dst_cap[r]): ZH_ERR_DST_TOO_SMALL for that range with out_len the size it
 * needs; none of its blocks is decoded and its slot is not written.  Slots must not overlap.  Of a slot only
 * [dst_off, dst_off + out_len) changes where the status is ZH_OK.
 * Two ranges that share a block decode it twice (no deduplication).  The blocks of all ranges together must stay
 * below 2^31, else ZH_ERR_ARGUMENT before anything is launched.
 * Blocks that lie wholly inside their range are decoded in place; the one or two its ends cut into go through
 * scratch the plan owns (bounded by ZH_SCRATCH_MB: beyond it, groups of ranges take turns) and are clipped into place.
 *
 * The plan runs with zh_plan_run(plan, d_src, d_dst) and is re-runnable; zh_plan_results returns n_ranges lengths
 * and statuses.  zh_plan_pack, zh_plan_unpack, zh_plan_set_src_lens_device, zh_plan_request_crc32 and
 * zh_plan_block_index return ZH_ERR_ARGUMENT for it. */
int zh_plan_uncompress_ranges(zh_ctx *ctx, size_t n_streams, const uint64_t *src_off, const uint64_t *src_len,
                              const zh_block_entry *index, const size_t *first,
                              size_t n_ranges, const uint64_t *range_stream, const uint64_t *range_off,
                              const uint64_t *range_len, const uint64_t *dst_off, const uint64_t *dst_cap,
                              zh_plan **out);
/* Host buffers in, library-allocated results out (zh_free), like zh_uncompress_batch: dsts[r] / dst_lens[r] where
 * statuses[r] is ZH_OK (a buffer of its own also for 0 bytes), NULL / 0 otherwise.  Of stream s only the bytes
 * [bit_off[k0] / 8, ceil(bit_off[k1+1] / 8)) that a range's blocks k0 .. k1 occupy are uploaded, spans of one stream
 * that overlap or touch once. */
int zh_uncompress_ranges(zh_ctx *ctx, const void *const *srcs, const size_t *lens, size_t n_streams,
                         const zh_block_entry *index, const size_t *first,
                         size_t n_ranges, const uint64_t *range_stream, const uint64_t *range_off,
                         const uint64_t *range_len, void **dsts, size_t *dst_lens, int32_t *statuses);
/* Counters of the context's last ranges call / plan run: bytes that went over the link (0 for a plan run: its streams
 * are on the device), blocks decoded in place, blocks decoded via scratch. */
int zh_debug_range_stats(zh_ctx *ctx, uint64_t *uploaded_bytes, uint64_t *blocks_in_place, uint64_t *blocks_via_scratch);

/* ------------------------------------------------------------------ *
 * BGZF, the blocked gzip of the SAM specification (section 4.1), as   *
 * written by bgzip and htslib: a series of gzip members of at most    *
 * 64 KiB, each with its total size in a `BC` extra subfield and its   *
 * CRC-32 and ISIZE in its trailer, closed by an empty 28-byte member. *
 * Any gunzip reads such a file; its index is in the file itself (a    *
 * walk over headers and trailers, nothing decoded), and a byte range  *
 * is verified by the checksums of the members it touches.             *
 * zh_uncompress* still rejects FEXTRA and multi-member input as the   *
 * reference does: these calls are the way to read and write BGZF.     *
 * Host buffers in, library-allocated results out (zh_free); statuses  *
 * per image or per range; the return value is ZH_OK unless the call   *
 * as a whole could not run, and then nothing is handed out.           *
 * ------------------------------------------------------------------ */
#define ZH_BGZF_BLOCK 65280     /* bgzip's payload per member (0xff00) */
#define ZH_BGZF_MAX_BLOCK 65505 /* largest payload whose stored form (5 + n) still fits a member */
#define ZH_BGZF_MAX_CDATA 65510 /* 65536 - 18 - 8 */

/* Member k starts at byte coff of the file and at byte uoff of the uncompressed data; a list is closed by one
 * entry: coff = the byte behind the last member that holds data or the EOF marker (= where the walk ended), uoff =
 * the total.  The virtual offset of htslib is coff << 16 | offset within the member. */
typedef struct zh_bgzf_entry {
  uint64_t coff, uoff;
} zh_bgzf_entry;

/* Image i = ceil(lens[i] / block_bytes) members and the EOF marker (a source of 0 bytes: the marker alone, as bgzip
 * writes it).  block_bytes: 0 means ZH_BGZF_BLOCK, else 1 .. ZH_BGZF_MAX_BLOCK (anything else: ZH_ERR_ARGUMENT).  A
 * bad level is ZH_ERR_INVALID_LEVEL for every image and the call, as in zh_compress_batch.  A member's CDATA is the
 * engine's raw deflate of its piece at `level` -- the bytes zh_compress gives for ZH_DF_DEFLATE -- except where that
 * stream is longer than ZH_BGZF_MAX_CDATA (the reference chooses stored blocks by a heuristic, never by size): such a
 * piece is written in its level-0 form, 5 + n bytes. */
int zh_bgzf_write_batch(zh_ctx *ctx, const void *const *srcs, const size_t *lens, size_t n, int level,
                        size_t block_bytes, void **dsts, size_t *dst_lens, int32_t *statuses);
/* The uncompressed data of every image.  The members are found by a walk from byte 0; the checks of the member at a
 * position, in this order, the first failure decides: fewer than 12 bytes left ZH_ERR_INVALID_BUFFER; ID bytes
 * ZH_ERR_GZIP_ID; CM != 8 ZH_ERR_UNSUPPORTED_METHOD; FLG & 0xe0 ZH_ERR_RESERVED_FLAGS; FLG != 4
 * ZH_ERR_UNSUPPORTED_FLAGS; 12 + XLEN beyond the image ZH_ERR_INVALID_BUFFER; subfields that do not tile XLEN or
 * hold no BC of two bytes ZH_ERR_BGZF_HEADER; BSIZE + 1 < 12 + XLEN + 8 ZH_ERR_BGZF_HEADER; the member beyond the
 * image ZH_ERR_INVALID_BUFFER; ISIZE > 65536 ZH_ERR_BGZF_HEADER.  The walk ends cleanly where a member ends with the
 * image (an image of 0 bytes: ZH_OK, 0 bytes); bytes behind an EOF marker are members like any others (cat a.gz
 * b.gz); a missing marker is no error (has_eof[i], if given: 1 when the walk ended cleanly and its last member is
 * byte for byte the marker).  Every member is decoded and settled: the decoder's status (more bytes than ISIZE:
 * ZH_ERR_SIZE), then its CRC-32 against the trailer (ZH_ERR_CHECKSUM), then its length against ISIZE (ZH_ERR_SIZE).
 * An image's status is that of its first failing member in file order, a header that fails counting at its own
 * position; such an image gives NULL / 0 and does not disturb its neighbours. */
int zh_bgzf_read_batch(zh_ctx *ctx, const void *const *images, const size_t *lens, size_t n, void **dsts,
                       size_t *dst_lens, int32_t *statuses, uint8_t *has_eof);
/* The walk alone: *index (zh_free) holds the lists of all images back to back, image i's entries are
 * index[first[i] .. first[i + 1]) (first: n + 1 values; an image that failed has none).  Nothing is decoded. */
int zh_bgzf_index_batch(zh_ctx *ctx, const void *const *images, const size_t *lens, size_t n, zh_bgzf_entry **index,
                        size_t *first, int32_t *statuses, uint8_t *has_eof);
/* Byte ranges of the uncompressed data, like pread and like zh_uncompress_ranges: range r reads bytes
 * [range_off[r], + range_len[r]) of image range_image[r]; it is clipped at the total, a range at or beyond it or of
 * length 0 gives 0 bytes and ZH_OK; range_image[r] >= n_images and NULL arrays are ZH_ERR_ARGUMENT; two ranges that
 * share a member decode it twice.  An index that cannot be right -- no entry, uoff[0] != 0, coff or uoff falling, a
 * member of more than 65536 bytes, coff beyond the image -- fails every range of THAT image with
 * ZH_ERR_INVALID_BUFFER.  Of an image only the bytes [coff[k0], coff[k1 + 1]) of the members k0 .. k1 a range
 * touches are uploaded, spans that overlap or touch once.  Every touched member's header is checked as above; it
 * must end at coff[k + 1] and its ISIZE be uoff[k + 1] - uoff[k], else ZH_ERR_INVALID_BUFFER; it is decoded whole
 * (into the range's slot when it lies inside the range, else into scratch of up to 64 KiB and clipped) and verified
 * by CRC-32 and ISIZE.  A range's status is that of its lowest failing member.  zh_debug_range_stats counts the
 * call's uploaded bytes and its members decoded in place / via scratch. */
int zh_bgzf_read_ranges(zh_ctx *ctx, const void *const *images, const size_t *lens, size_t n_images,
                        const zh_bgzf_entry *index, const size_t *first, size_t n_ranges,
                        const uint64_t *range_image, const uint64_t *range_off, const uint64_t *range_len,
                        void **dsts, size_t *dst_lens, int32_t *statuses);

/* ------------------------------------------------------------------ *
 * Any gzip file (RFC 1952): several members back to back (cat a.gz    *
 * b.gz, appended logs, pigz -i, .warc.gz), FEXTRA, FNAME, FCOMMENT    *
 * and FHCRC fields -- what every gunzip reads.  zh_uncompress* keeps  *
 * the reference's contract (one member, no FEXTRA, the trailer the    *
 * image's last eight bytes); this call is the way to read the rest.   *
 * A plain member does not say how long it is: every position that     *
 * could start one is sized on the device at once, and the chain from  *
 * byte 0 is proved afterwards.  Host buffers in, library-allocated    *
 * results out (zh_free), as in zh_bgzf_read_batch.                    *
 * ------------------------------------------------------------------ */
/* One reached member.  coff, cdata_off, cdata_len: in the image -- its first header byte, its first deflate byte, its
 * deflate bytes (whole bytes); uoff, ulen: in the image's uncompressed data; crc, isize: its trailer; mtime, flg, xfl,
 * os: its header, reported and not judged; the optional fields' places count from coff, lengths without the closing
 * NUL, 0 / 0 for a field that is absent (FEXTRA's are the bytes behind XLEN; subfields are not interpreted). */
typedef struct zh_gzip_member {
  uint64_t coff, cdata_off, cdata_len;
  uint64_t uoff, ulen;
  uint32_t crc, isize, mtime;
  uint8_t flg, xfl, os, pad;
  uint32_t extra_off, extra_len, name_off, name_len, comment_off, comment_len;
} zh_gzip_member;

/* The uncompressed data of every image: its members' data back to back.  dsts / dst_lens may both be NULL: the members
 * are still decoded and verified on the device, no data comes down.  members / first (n + 1 values) may both be NULL;
 * else *members (zh_free) holds the lists of all images back to back, image i's members are members[first[i] ..
 * first[i + 1]) (an image that failed has none).  NULL images / lens / statuses with n > 0, or one of a pair without
 * the other: ZH_ERR_ARGUMENT.  The return value is ZH_OK unless the call as a whole could not run; an image that
 * failed gives NULL / 0 and does not disturb its neighbours.
 * The member at position p of an image, in this order, the first failure decides:
 *   1. fewer than 18 bytes left: ZH_ERR_INVALID_BUFFER;
 *   2. ID bytes: ZH_ERR_GZIP_ID;  3. CM != 8: ZH_ERR_UNSUPPORTED_METHOD;  4. FLG & 0xe0: ZH_ERR_RESERVED_FLAGS;
 *   5. FEXTRA: 12 + XLEN beyond the image ZH_ERR_INVALID_BUFFER;
 *   6. FNAME, then FCOMMENT: no NUL before the image's end ZH_ERR_INVALID_BUFFER;
 *   7. FHCRC: its two bytes beyond the image ZH_ERR_INVALID_BUFFER (it is verified below);
 *   8. a header of more than 4 GiB (the fields' places are 32 bits wide): ZH_ERR_INVALID_BUFFER.
 * The deflate stream runs from cdata_off to its own final block: the decoder's statuses are those of
 * zh_uncompress(.., ZH_DF_DEFLATE), its input is bounded by the image's end minus 8, and the member ends at the final
 * block's last byte plus the 8 trailer bytes (beyond the image: ZH_ERR_INVALID_BUFFER).  Where a member ends, the
 * image ends too (a clean end), or all remaining bytes are zero (a clean end: tape and block padding, as gzip and
 * Python's gzip accept it), or a member must start there and the checks above give the status.  An image of 0 bytes
 * gives ZH_OK, 0 bytes and 0 members; zeros alone are no member (ZH_ERR_GZIP_ID from 18 bytes on).
 * Every reached member is settled by the first of these that applies: its header's status; the decoder's; FHCRC, when
 * present, against the low 16 bits of the CRC-32 of the header bytes before it (ZH_ERR_CHECKSUM); the CRC-32 of its
 * data against the trailer's (ZH_ERR_CHECKSUM); ulen mod 2^32 against ISIZE (ZH_ERR_SIZE); what stands behind it.  An
 * image's status is that of its first failing member in file order.
 * The sizing of candidates that are no members is bounded: a workgroup of the pass stops once the pass's workgroups
 * together have paid ZH_GZIP_SPEC_BYTES input bytes (the environment; default 2 x the call's image bytes + 64 MiB).  A
 * workgroup pays, and looks, where it reads a block header or stages a superchunk, so the pass reads at most the budget
 * plus what every workgroup resident on the device consumes between two looks: 64 KiB, 65540 bytes for a full stored
 * block.  The members the chain still needs are then sized one round of the chain's ends at a time -- the same
 * results.  The searches for the NUL of FNAME / FCOMMENT pay into the same sum, 4 KiB at a time: an image without a
 * zero byte cannot buy more header reading than that either. */
int zh_gzip_read_batch(zh_ctx *ctx, const void *const *images, const size_t *lens, size_t n, void **dsts,
                       size_t *dst_lens, int32_t *statuses, zh_gzip_member **members, size_t *first);
/* The last zh_gzip_read_batch of the context: the positions sized as members, the input bytes the budgeted sizing pass
 * consumed, the rounds that sized chain ends the budget had left out. */
int zh_debug_gzip_stats(zh_ctx *ctx, uint64_t *candidates, uint64_t *speculative_bytes, uint64_t *frontier_rounds);

/* ------------------------------------------------------------------ *
 * Seek indexes for FOREIGN deflate streams (zlib, pigz, gzip, zip     *
 * entries: every block reaches up to 32 KiB back into the one before) *
 * -- the idea of zlib's zran.c: decode the stream once, keep at       *
 * chosen block boundaries the bit position, the output position and   *
 * the 32 KiB of output before it; from then on a byte range needs the *
 * compressed bytes of the intervals it touches and their windows, and *
 * every interval decodes on its own.  The index is built from a fully *
 * decoded, container-verified stream and carries a CRC-32 per         *
 * interval: every range read is verified.                             *
 * ------------------------------------------------------------------ */
/* The index of one stream is one flat little-endian blob (library-allocated, zh_free; it may be written to disk):
 *   zh_seek_header, 64 bytes | n_points records of zh_seek_point, 32 bytes each | the window store, window_bytes.
 * Point k: the deflate block whose header's first bit is bit_off, counted from the first byte of the buffer (container
 * header included, as in zh_block_entry), begins at byte out_off of the uncompressed data; the win_len = min(out_off,
 * 32768) bytes of output before it lie at win_off of the window store (a multiple of 16; every window is padded with
 * zeros to a multiple of 16); crc32 is the CRC-32 of the uncompressed bytes [out_off, next point's out_off).  The last
 * point is the closing entry: the bit just behind the final block's end-of-block code, `total`, win_len 0, crc32 0.
 * Which block boundaries become points: point 0 is the first block (out_off 0, no window); going through the later
 * block starts in stream order, a block start becomes a point when its out_off minus the last point's out_off is at
 * least `span` (of several empty blocks at one out_off, the first that qualifies).  Points lie at block boundaries
 * ONLY: a stream of one 4 MiB block has point 0 and the closing entry whatever the span.  The blob is pinned by this
 * rule: the same stream and span give the same bytes. */
#define ZH_SEEK_MAGIC "ZHSKIDX1"
#define ZH_SEEK_VERSION 1u
#define ZH_SEEK_WINDOW 32768u
#define ZH_SEEK_DEFAULT_SPAN 1048576u /* span 0 (zran's default) */
typedef struct zh_seek_header {
  char magic[8];         /* ZH_SEEK_MAGIC */
  uint32_t version;      /* ZH_SEEK_VERSION */
  uint32_t data_format;  /* resolved: ZH_DF_ZLIB, ZH_DF_GZIP or ZH_DF_DEFLATE */
  uint64_t src_len;      /* bytes of the compressed buffer */
  uint64_t total;        /* bytes of the uncompressed data */
  uint64_t span;         /* as resolved (never 0) */
  uint64_t n_points;     /* closing entry included */
  uint64_t window_bytes; /* bytes of the window store */
  uint64_t reserved;     /* 0 */
} zh_seek_header;
typedef struct zh_seek_point {
  uint64_t bit_off, out_off, win_off;
  uint32_t win_len, crc32;
} zh_seek_point;

/* One index per stream (indexes[i] / index_lens[i], zh_free), and with dsts / dst_lens (both or neither) the decoded
 * data as well (otherwise it is not downloaded).  statuses[i] is what zh_uncompress_batch gives stream i: container
 * header, CRC-32 / Adler-32 and ISIZE are all checked; an index exists only for a stream that decodes with ZH_OK, a
 * bad stream gives NULL / 0 and does not disturb its neighbours.  span: 0 means ZH_SEEK_DEFAULT_SPAN, otherwise at
 * least ZH_SEEK_WINDOW (anything else: ZH_ERR_ARGUMENT for the call).  n == 0 launches nothing.  Every stream takes
 * the one-workgroup-a-stream decoder, which records the points as it goes (large single streams are not decoded
 * segment-wise here). */
int zh_seek_index_batch(zh_ctx *ctx, const void *const *srcs, const size_t *lens, size_t n, int data_format,
                        uint64_t span, void **indexes, size_t *index_lens, void **dsts, size_t *dst_lens,
                        int32_t *statuses);
/* Byte ranges of the uncompressed data of streams with seek indexes, like pread and word for word like
 * zh_uncompress_ranges: a range is clipped at `total`; range_off at or beyond it, or range_len 0, gives 0 bytes and
 * ZH_OK and touches nothing; range_off + range_len beyond 2^64 is clipped; range_stream[r] >= n_streams and NULL
 * arrays are ZH_ERR_ARGUMENT; two ranges that share an interval decode it twice.
 * A blob that cannot be right fails every range of THAT stream, and no other, with ZH_ERR_INVALID_BUFFER: wrong magic
 * or version, a length that does not match its own counts, src_len != lens[s], fewer than two points, out_off[0] != 0,
 * bit_off not strictly rising or at or beyond 8 * src_len (beyond, for the closing entry), out_off falling, win_len !=
 * min(out_off, 32768), a window outside the store or not at a multiple of 16, an interval that promises more than
 * 1032 * (its compressed bytes) + 64 bytes.
 * Of stream s only the bytes [bit_off[k0] / 8, ceil(bit_off[k1 + 1] / 8)) of the intervals k0 .. k1 a range touches
 * are uploaded -- spans of one stream that overlap or touch once -- and the windows of exactly those intervals;
 * zh_debug_range_stats reports those bytes (spans plus windows), 0 intervals in place and the intervals decoded.
 * Every touched interval decodes on its own into a scratch slot [window | output] (scratch bounded by
 * ZH_SCRATCH_MB: groups of ranges take turns): it starts at bit_off[k] with the window as its history -- a match that
 * reaches beyond the window is ZH_ERR_INVALID_BUFFER --, and stops at a block boundary at bit_off[k + 1] (a block
 * boundary beyond it, or a final block that ends elsewhere: ZH_ERR_INVALID_BUFFER).  Verified per interval, in this
 * order: the decoder's status; exactly out_off[k + 1] - out_off[k] bytes made (else ZH_ERR_INVALID_BUFFER); their
 * CRC-32 equal to the point's (else ZH_ERR_CHECKSUM).  A range's status is that of its lowest failing interval, its
 * length then 0; ranges that touch no bad interval succeed.  The container's header and trailer are not looked at:
 * the build verified them. */
int zh_seek_read_ranges(zh_ctx *ctx, const void *const *srcs, const size_t *lens, size_t n_streams,
                        const void *const *indexes, const size_t *index_lens, size_t n_ranges,
                        const uint64_t *range_stream, const uint64_t *range_off, const uint64_t *range_len,
                        void **dsts, size_t *dst_lens, int32_t *statuses);

/* ------------------------------------------------------------------ *
 * Resumable uncompress: streams decoded as their bytes arrive.        *
 * Host buffers in, library-allocated results out (zh_free); statuses  *
 * per stream; the return value is ZH_OK unless the call as a whole    *
 * could not run.                                                      *
 * ------------------------------------------------------------------ */
/* What carries a stream from one call to the next is one flat little-endian blob (library-allocated, zh_free; the
 * caller keeps it and hands it back): this header and the last win_len bytes made.  The same stream, the same
 * chunking and the same max_out give the same bytes. */
#define ZH_RESUME_MAGIC "ZHRESUM1"
#define ZH_RESUME_VERSION 1u
typedef struct zh_resume_header { /* 64 bytes, little endian; win_len bytes of window follow */
  char magic[8];
  uint32_t version;
  uint32_t data_format; /* resolved: ZH_DF_ZLIB, ZH_DF_GZIP or ZH_DF_DEFLATE */
  uint32_t phase;       /* 1: the next bit is a block header; 2: the final block is done, the trailer is due */
  uint32_t bit_skip;    /* 0..7: that bit's place in the first byte of the next call's input (0 in phase 2) */
  uint64_t total_in;    /* bytes consumed by all calls so far */
  uint64_t total_out;   /* bytes made by all calls so far */
  uint32_t check;       /* running CRC-32 (gzip) / Adler-32 (zlib) of those bytes; 0 for raw deflate */
  uint32_t win_len;     /* min(total_out, 32768): the last win_len bytes made */
  uint64_t reserved[2]; /* 0 */
} zh_resume_header;
enum { ZH_RESUME_DONE = 0, ZH_RESUME_NEED_INPUT = 1, ZH_RESUME_NEED_OUTPUT = 2 };

/* One call decodes, for every stream i, as many WHOLE deflate blocks as srcs[i] holds and max_out[i] allows: every
 * block whose last bit lies inside the input and whose output, added to what the call has made already, stays at or
 * below max_out[i]; it stops at the first block that fails either test (empty blocks count as progress).  For a new
 * stream (states[i] NULL; states NULL: all of them) srcs[i] starts at the container's header and data_format is
 * resolved as in zh_uncompress_batch -- with four bytes in hand --; otherwise srcs[i] starts at the byte the call
 * before left, srcs_prev[i] + consumed_prev[i], the unconsumed tail followed by what arrived since, the first block
 * header at bit bit_skip of byte 0, and the format is the state's.  dsts[i] / dst_lens[i] (zh_free; NULL for no
 * bytes) hold exactly the delivered blocks' bytes; consumed[i] is the index of the byte that holds the next block's
 * first bit (that byte is consumed only when bit_skip is 0); new_states[i] / new_state_lens[i] (zh_free) the state to
 * come back with.  why[i], the earliest event in stream order deciding (one exception: the output is written in rounds of
 * up to 64 bytes, and while a stream has made fewer than 32768 bytes a distance beyond the window anywhere in a round
 * is ZH_ERR_INVALID_BUFFER even where the budget was passed a token earlier in that round):
 *   ZH_RESUME_DONE         the final block is delivered and the trailer verified -- CRC-32 (ZH_ERR_CHECKSUM) and
 *                          ISIZE (ZH_ERR_SIZE), or Adler-32, nothing for raw deflate --; consumed[i] is the index just
 *                          behind the trailer (a following member's bytes are not looked at), new_states[i] is NULL;
 *   ZH_RESUME_NEED_INPUT   the input ended inside a block, a block header or the trailer (phase 2);
 *   ZH_RESUME_NEED_OUTPUT  the next block would pass max_out[i].
 * The container's header: the checks and statuses of zh_uncompress_batch (no FEXTRA, no preset dictionary; FHCRC is
 * skipped), made once the header is whole: ten bytes of a gzip member and its name, comment and header CRC, two bytes
 * of a zlib stream.  A header that the end of the input cuts short is ZH_RESUME_NEED_INPUT with consumed[i] 0 and no
 * state: come back with more bytes and a NULL state.
 * Soundness: a prefix of a stream that zh_uncompress_batch decodes with ZH_OK never yields an error, at any cut: no
 * check is decided by a bit at or beyond 8 * lens[i].  A field, a code or a token that the end of the input cuts, a
 * stored block whose bytes are not all there, and a pattern that no code claims with fewer bits behind it than the
 * longest code may have (7 in a dynamic header's code-length code, 15 elsewhere) are ZH_RESUME_NEED_INPUT.
 * last[i] != 0 (last NULL: none) promises that no more input exists: the end of the input is the end of the stream,
 * the checks read zeros behind it as zh_uncompress_batch's do, and where ZH_RESUME_NEED_INPUT would be answered the
 * status is the whole call's: ZH_ERR_END_OF_BUFFER inside a block, what the zeros make of a block header
 * (ZH_ERR_INVALID_BUFFER at a block boundary), ZH_ERR_CHECKSUM inside the trailer; a new stream's header is judged
 * with zh_uncompress_batch's own length rules (those rules speak of the whole stream's length -- more than 18 bytes of
 * gzip, 6 of zlib --: a shorter stream that comes in several calls ends with the decoder's or the trailer's status
 * instead).  A definite error may surface in an earlier call, with the same code; the blocks that EARLIER calls made
 * whole were delivered by then.  The call that meets the error delivers nothing, the good blocks in front of the
 * damaged one included: who wants what was decodable before the damage feeds smaller pieces or a smaller max_out.
 * statuses[i] != ZH_OK gives stream i no output, no state and consumed[i] 0, and never disturbs its neighbours.  A
 * match that reaches beyond the window is ZH_ERR_INVALID_BUFFER.  A state that cannot be right -- magic, version,
 * format, phase outside 1..2, bit_skip > 7 or non-zero in phase 2, win_len != min(total_out, 32768), a length other
 * than 64 + win_len, reserved != 0 -- fails its stream with ZH_ERR_INVALID_BUFFER before anything is uploaded.
 * ZH_ERR_ARGUMENT for the call: NULL arrays; a NULL source with a non-zero length; a NULL state with a non-zero
 * length; max_out[i] == 0; state_lens without states or states without state_lens.  n == 0 launches nothing.  A
 * call that fails as a whole hands nothing out: every dsts[i] and new_states[i] is NULL.
 * A call makes progress only when the input holds a whole block and max_out its output (zlib's blocks are tens of
 * KiB, this library's up to 4 MiB of data); resuming inside a block is not offered.  One stream decodes on one
 * workgroup: many streams side by side is the case this serves.  Scratch is bounded by ZH_SCRATCH_MB, groups of
 * streams taking turns. */
int zh_uncompress_resume_batch(zh_ctx *ctx, const void *const *srcs, const size_t *lens, size_t n, int data_format,
                               const void *const *states, const size_t *state_lens, /* NULL entry: a new stream */
                               const uint64_t *max_out, const uint8_t *last,        /* last: NULL = none */
                               void **dsts, size_t *dst_lens, size_t *consumed,
                               void **new_states, size_t *new_state_lens, int32_t *why, int32_t *statuses);

/* ------------------------------------------------------------------ *
 * Streaming compress: streams fed piece by piece, flushed, finished.  *
 * Host buffers in, library-allocated results out (zh_free); statuses  *
 * per stream; the return value is ZH_OK unless the call as a whole    *
 * could not run.                                                      *
 * ------------------------------------------------------------------ */
/* The reference runs its matcher once per deflate block, and no match crosses a block start (above: the block-parallel
 * form).  A stream compressed piece by piece is therefore the bit-concatenation of the pieces' own raw-deflate streams
 * with BFINAL cleared on all but the last: every byte of it can be held against the reference.  What carries a stream
 * from one call to the next is this 64-byte little-endian blob (library-allocated, zh_free; the caller keeps it and
 * hands it back).  No history survives a call: a piece's matches reach no further back than its own first byte. */
enum { ZH_FLUSH_BLOCK = 0, ZH_FLUSH_SYNC = 1, ZH_FLUSH_FINISH = 2 };
#define ZH_STREAM_MAGIC "ZHCSTRM1"
#define ZH_STREAM_VERSION 1u
typedef struct zh_stream_state { /* 64 bytes, little endian, nothing follows */
  char magic[8];
  uint32_t version;     /* 1 */
  uint32_t data_format; /* ZH_DF_ZLIB, ZH_DF_GZIP or ZH_DF_DEFLATE */
  int32_t level;        /* fixed at the first call */
  uint32_t block_bytes; /* fixed at the first call */
  uint32_t phase;       /* 1: header written, stream open */
  uint32_t pend_bits;   /* 0..7 bits made but not yet delivered */
  uint32_t pend_byte;   /* those bits, low first; the rest 0 */
  uint32_t check;       /* running CRC-32 (gzip) / Adler-32 (zlib) of the input; 0 for raw deflate */
  uint64_t total_in;    /* input consumed by all calls so far */
  uint64_t total_out;   /* compressed bytes delivered by all calls so far, header included */
  uint64_t reserved;    /* 0 */
} zh_stream_state;

/* WHAT THE BYTES ARE.  The output of calls 1..m of one stream, concatenated, is a bit string (deflate's order: the low
 * bit of a byte first):
 *  1. New stream (states[i] NULL; states NULL: all of them): the container header exactly as zh_compress of this
 *     context writes it for this level and format -- ten bytes of gzip plus the name zh_set_gzip_fname_len asks for and
 *     its NUL, two bytes of zlib, nothing for raw deflate.  level, data_format and block_bytes (0: 4 MiB) are those of
 *     the call; a resumed stream takes all three from its state.
 *  2. Each call with lens[i] > 0, or with ZH_FLUSH_FINISH: the bits [0, end) of
 *       R = zh_compress_blocks(piece, level, ZH_DF_DEFLATE, block_bytes),
 *     end being the closing index entry's bit_off, with the BFINAL bit of the last block (the last index entry before
 *     the closing one) cleared unless the call is ZH_FLUSH_FINISH.  They are placed behind the k = pend_bits pending
 *     bits as follows; let p be the bit_off of the first STORED block of R (BTYPE 00), if there is one.
 *       - Without a stored block every bit moves up by k.
 *       - With one, bits [0, p + 3) move up by k, and zero bits follow up to the next byte boundary of the
 *         DESTINATION.  Everything from source byte ceil((p + 3) / 8) on (LEN, NLEN, data, all later blocks) follows
 *         at destination byte ceil((p + k + 3) / 8): a whole-byte move of 0 or 1.
 *       - A stored block aligns source and destination alike, so every later stored block keeps its own padding:
 *         there are only ever these two regimes.
 *  3. ZH_FLUSH_BLOCK with an empty piece: nothing.
 *  4. ZH_FLUSH_FINISH with an empty piece: the block that zh_compress(empty, level, ZH_DF_DEFLATE) makes
 *     (01 00 00 ff ff; at HuffmanOnly the coded block 03 00), placed by the same rule.
 *  5. ZH_FLUSH_SYNC: then three zero bits, zero bits to the byte boundary, and 00 00 FF FF (an empty stored block).
 *     After it pend_bits is 0, and everything delivered so far decodes to everything fed so far.
 *  6. ZH_FLUSH_FINISH: zero bits to the byte boundary, then the trailer over the whole input -- gzip: CRC-32 and
 *     total_in mod 2^32, little endian; zlib: Adler-32, big endian; raw deflate: nothing.  The stream is over:
 *     new_states[i] is NULL.
 *  7. Delivery: a call delivers the whole bytes of what exists so far (dsts[i] / dst_lens[i], zh_free; NULL for no
 *     bytes); the up to 7 bits left over go into the state, not into the output.
 * Identity: pieces that are multiples of block_bytes fed with ZH_FLUSH_BLOCK, the last piece with ZH_FLUSH_FINISH,
 * give byte for byte zh_compress_blocks(whole, level, data_format, block_bytes) -- with block_bytes 0 the reference's
 * own compress(whole): a file larger than memory gets the reference's bytes.  (At level 0 the unit is 65535 bytes: the
 * reference cuts stored chunks there whatever the block size.)  After zh_set_l1_parse(ctx, 1) R is that mode's
 * stream: the rule is unchanged and the bytes are valid, but not the reference's.
 * flush[i] is one of ZH_FLUSH_* (flush NULL: all ZH_FLUSH_SYNC).  One status per stream; statuses[i] != ZH_OK gives
 * stream i no output and no state and never disturbs its neighbours.  A state that cannot be right -- magic, version,
 * format, level outside -2..9, block_bytes not a multiple of 32768 in 32768..4194304, phase != 1, pend_bits > 7, bits of
 * pend_byte at or above pend_bits, reserved != 0, a length other than 64 -- fails its stream with
 * ZH_ERR_INVALID_BUFFER before anything is uploaded.  ZH_ERR_ARGUMENT for the call: NULL arrays; a NULL source with a
 * non-zero length; a NULL state with a non-zero length; flush[i] > 2; state_lens without states or states without
 * state_lens; a bad level, format (ZH_DF_DETECT is not a format to write) or block_bytes when any stream is new.
 * n == 0 launches nothing.  A call that fails as a whole hands nothing out: every dsts[i] and new_states[i] is NULL.
 * Streams of one level and block size share a compress plan; scratch is bounded by ZH_SCRATCH_MB, groups of streams
 * taking turns.  Small pieces pay for it in ratio (every piece starts without history and with codes of its own) and
 * in speed (a call has a plan's fixed cost): DESIGN.md 4.19 has the measurements. */
int zh_compress_stream_batch(zh_ctx *ctx, const void *const *srcs, const size_t *lens, size_t n,
                             int level, int data_format, size_t block_bytes,      /* for new streams; 0 = 4 MiB */
                             const void *const *states, const size_t *state_lens, /* NULL entry: a new stream */
                             const uint8_t *flush,                                /* per stream; NULL = all SYNC */
                             void **dsts, size_t *dst_lens, void **new_states, size_t *new_state_lens,
                             int32_t *statuses);

/* ------------------------------------------------------------------ *
 * ZIP archives as batch clients of the codec. *
 * Record parsing / assembly of src/zippy/ziparchives.nim on the host, *
 * every entry's deflate stream and CRC-32 in ONE GPU batch.  The file *
 * system side of extractAll (ziparchives.nim:374-453) stays with the  *
 * caller.                                                             *
 * ------------------------------------------------------------------ */
typedef struct zh_zip_reader zh_zip_reader;
typedef struct zh_zip_entry {
  const char *path;           /* UTF-8, not NUL-terminated; CP437 names converted (ziparchives.nim:108-160) */
  size_t path_len;
  int is_directory;           /* ziparchives.nim:352-359 */
  uint64_t header_offset;     /* of the local file header in the image */
  uint64_t compressed_size, uncompressed_size;
  uint32_t crc32;
  uint32_t unix_mode;         /* external attributes >> 16 (parseFilePermissions' input) */
} zh_zip_entry;

/* openZipArchive(zipPath) -- ziparchives.nim:183-372 -- on a memory image, which stays borrowed
 * until zh_zip_close.  Entries keep central-directory order. */
int zh_zip_open(const void *archive, size_t len, zh_zip_reader **out);
void zh_zip_close(zh_zip_reader *reader);
size_t zh_zip_num_entries(const zh_zip_reader *reader);
int zh_zip_entry_at(const zh_zip_reader *reader, size_t i, zh_zip_entry *out);
int zh_zip_find(const zh_zip_reader *reader, const char *path, size_t path_len, size_t *index);
/* extractFile(reader, path) -- ziparchives.nim:39-93 -- for n records at once; statuses[k] is
 * the outcome of record indices[k], dsts[k] library-allocated (zh_free). */
int zh_zip_extract_batch(zh_ctx *ctx, const zh_zip_reader *reader, const size_t *indices, size_t n,
                         void **dsts, size_t *dst_lens, int32_t *statuses);
/* createZipArchive(entries: OrderedTable[string, string]) -- ziparchives.nim:455-634.  Entries in
 * insertion order (the archive lists them last to first, as the reference does); dos_time /
 * dos_date = msdos(getTime()) (ziparchives.nim:475-493), taken from the caller so that the
 * call is a pure function. */
int zh_zip_create(zh_ctx *ctx, const char *const *paths, const size_t *path_lens,
                  const void *const *contents, const size_t *content_lens, size_t n,
                  uint16_t dos_time, uint16_t dos_date, void **archive, size_t *archive_len);

/* openZipArchive + the extraction loop of extractAll (ziparchives.nim:183-372, :374-453 without the file system) for
 * n_zip images per call.  readers[t] is an ordinary reader -- zh_zip_num_entries / zh_zip_entry_at / zh_zip_find /
 * zh_zip_extract_batch / zh_zip_close --, NULL when archive t did not open; the image stays borrowed until close, the
 * extracted bytes are the reader's.  statuses[t] is the first of:
 *  1. what zh_zip_open(images[t], lens[t], ..) returns for that image alone (the reader is NULL then);
 *  2. ZH_ERR_UNSAFE_PATH if any record's path is absolute, starts with ../ or ..\ or contains /../ or \..\
 *     (verifyPathIsSafeToExtract; extractAll checks every path before it extracts anything): the reader is returned,
 *     nothing was extracted, and zh_zip_entry_data reports ZH_ERR_UNSAFE_PATH for every file record;
 *  3. the status of the first FILE record, in directory order, whose extraction failed: the reader and every other
 *     entry's data are returned.
 * The return value is a call-level error only: NULL arrays, an image that is NULL with a non-zero length, a missing
 * ctx, allocation, device; more than 2^32 - 2 walk nodes (directory bytes) or records in one call: ZH_ERR_ARGUMENT
 * before anything is launched.  A bad archive never changes another archive's reader, statuses or bytes; n_zip == 0
 * launches nothing.
 * The host only finds each directory (the end records); the images are uploaded once, the directory walk (pointer
 * doubling over the directory's bytes), every check of openZipArchive's loop body and of extractFile's local header,
 * the copies of stored entries and every CRC-32 verdict run on the device, and ONE uncompress plan decodes every
 * deflated entry of the call from its place in the uploaded image (csrc/zh_zip_open_batch.hip). */
int zh_zip_open_all_batch(zh_ctx *ctx, const void *const *images, const size_t *lens, size_t n_zip,
                          zh_zip_reader **readers, int32_t *statuses);
/* Contents of a reader made by the call above: all extracted files of the archive in one block owned by the reader,
 * every entry 8-byte aligned, in directory order (NULL / 0 for a zh_zip_open reader, and when nothing was extracted). */
const void *zh_zip_data(const zh_zip_reader *reader, size_t *len);
/* Entry i of such a reader: *status is, for a file record, exactly what zh_zip_extract_batch reports for that index
 * (ZH_ERR_ARCHIVE_EOF, ZH_ERR_ZIP_FILE_HEADER, ZH_ERR_ZIP_METHOD, ZH_ERR_ZIP_CRC or a decoder status) and data / len
 * byte-identical to its output (NULL / 0 unless ZH_OK); for a directory record ZH_OK with length 0 (extractAll only
 * calls createDir for them: their local headers are not read).  The data lie inside zh_zip_data()'s block, except for
 * an entry whose directory understated its size: that one was decoded again on its own and has a buffer of its own
 * (the reader's as well).  A reader made by zh_zip_open, a NULL pointer or an index out of range: ZH_ERR_ARGUMENT. */
int zh_zip_entry_data(const zh_zip_reader *reader, size_t i, const void **data, size_t *len, int32_t *status);

/* ZipArchive.open(stream / path) -- ziparchives_v1.nim:105-349 openStreamImpl -- for n_zip images per call.  This is
 * not openZipArchive under another name: it never looks for the end record.  It starts at byte 0 and walks the whole
 * image record by record -- local headers with their data, central records, the end record --, decoding and verifying
 * every entry on the way.  statuses[t] is the outcome of openStreamImpl on image t alone, the first check that fails:
 *   at `pos` (0 at first): pos + 4 > len: ZH_ERR_ARCHIVE_EOF (failEOF); a signature that is none of the three:
 *     ZH_ERR_ZIP_OPEN (:328-329);
 *   50 4b 03 04 (:120-225): pos + 30 > len: ZH_ERR_ARCHIVE_EOF; flag bit 2: ZH_ERR_ZIP_DATA_DESCRIPTOR; flag bit 3:
 *     ZH_ERR_ZIP_DEFLATE64; a method outside {0, 8}: ZH_ERR_ZIP_METHOD; name + extra, then the data (the 32-bit
 *     compressed size) beyond the image: ZH_ERR_ARCHIVE_EOF; method 8: the status zh_uncompress_batch(.., ZH_DF_DEFLATE)
 *     gives those bytes; the CRC-32 of the contents against the header's: ZH_ERR_ZIP_CRC; only then their length
 *     against the header's uncompressed size: ZH_ERR_ZIP_SIZE.  The key is the name with every \ replaced by /
 *     (toUnixPath); contents[key] = entry replaces the value of an earlier equal key and keeps that key's place;
 *   50 4b 01 02 (:227-293): pos + 46 > len, then name + extra + comment beyond the image: ZH_ERR_ARCHIVE_EOF; the RAW
 *     name is not a key inserted so far: ZH_ERR_ZIP_OPEN; else the entry's is_directory = external attributes & 0x10,
 *     unix_mode = external attributes >> 16 (a later central record of the same name overwrites both);
 *   50 4b 05 06 (:295-326): pos + 22 > len, then the comment beyond the image: ZH_ERR_ARCHIVE_EOF; else ZH_OK, and
 *     nothing behind it is looked at.
 * readers[t] is NULL unless statuses[t] is ZH_OK (the reference leaves a half-filled table behind its exception; the
 * library returns none).  A reader's entries are the table's keys in first-insertion order, each with the value of
 * its last local record: zh_zip_num_entries / zh_zip_entry_at (header_offset, both sizes and the CRC of that local
 * record; is_directory and unix_mode as above, 0 without a central record; path = the key) / zh_zip_find (on the key) /
 * zh_zip_data / zh_zip_entry_data (always ZH_OK with the bytes, a directory's too: v1 keeps them) / zh_zip_close work
 * on it; zh_zip_extract_batch returns ZH_ERR_ARGUMENT (every entry is extracted already).  The image stays borrowed
 * until zh_zip_close.
 * The return value is a call-level error only: NULL arrays, an image that is NULL with a non-zero length, a missing
 * ctx, allocation, device; images that could hold more than 2^32 - 2 walk nodes (signatures: one in four bytes, plus
 * one node an image) or records in one call: ZH_ERR_ARGUMENT before anything is launched.  A bad image never changes
 * another image's reader, status or bytes; n_zip == 0 launches nothing.
 * The images are uploaded once; a signature scan over every image byte, the walk over its hits (pointer doubling),
 * every header check, the copies of stored entries and every CRC-32 / size verdict run on the device, and ONE
 * uncompress plan decodes every deflated local record of the call from its place in the uploaded image; the host
 * inserts the tables (csrc/zh_zip_read_batch.hip). */
int zh_zip_read_batch(zh_ctx *ctx, const void *const *images, const size_t *lens, size_t n_zip,
                      zh_zip_reader **readers, int32_t *statuses);
/* Entry i of a reader made by zh_zip_read_batch: the raw DOS time and date words of its local record (:128-129; the
 * conversion to times.Time, :161-179, is in the caller's zone and stays with the caller) and whether a central record
 * named the entry (without one, permissions stay unset).  Any other reader, a NULL pointer or an index out of range:
 * ZH_ERR_ARGUMENT. */
int zh_zip_entry_v1(const zh_zip_reader *reader, size_t i, uint16_t *dos_time, uint16_t *dos_date,
                    int *in_directory);

/* ------------------------------------------------------------------ *
 * Tarballs: extractAll of src/zippy/tarballs.nim *
 * without its file-system half.  A .tar.gz is ONE foreign gzip member *
 * -- one decoder, no parallelism to offer; the GPU still does the     *
 * inflate + CRC-32, with ISIZE as the output size (trustSize).        *
 * ------------------------------------------------------------------ */
typedef struct zh_tar_reader zh_tar_reader;
typedef struct zh_tar_entry {
  const char *path;      /* prefix / name, or the preceding 'L' block's long name */
  size_t path_len;
  const char *linkname;  /* symlinks (typeflag '2') */
  size_t linkname_len;
  char typeflag;         /* '0' or '\0' file, '5' directory, '2' symlink */
  uint32_t mode;
  int64_t mtime;
  uint64_t offset, size; /* the entry's bytes inside zh_tar_data() */
} zh_tar_entry;

/* image: the bytes of a .tar.gz (decoded here; ctx required) or of a .tar (borrowed until close;
 * ctx may be NULL).  Header walk and checks: tarballs.nim:61-124. */
int zh_tar_open(zh_ctx *ctx, const void *image, size_t len, zh_tar_reader **out);
void zh_tar_close(zh_tar_reader *reader);
size_t zh_tar_num_entries(const zh_tar_reader *reader);
int zh_tar_entry_at(const zh_tar_reader *reader, size_t i, zh_tar_entry *out);
const void *zh_tar_data(const zh_tar_reader *reader, size_t *len);

/* extractAll of tarballs.nim:26-124 (without the file system) for n_tar images per call.
 * readers[t]: an ordinary reader -- zh_tar_num_entries / zh_tar_entry_at / zh_tar_data / zh_tar_close --, NULL when
 * statuses[t] != 0.  statuses[t] is exactly what zh_tar_open(ctx, images[t], lens[t], ..) returns for
 * that image alone; a bad image never changes the others.  The return value is a call-level error only:
 * NULL arrays, an image that is NULL with a non-zero length, allocation, device.
 * A plain .tar image is borrowed until its reader is closed; the uncompressed image of a .tar.gz is owned by its
 * reader.  ctx is required (the header walk runs on the device for plain images too); n_tar == 0 launches nothing.
 * Every gzip member of the call is decoded by one uncompress plan, with ISIZE as the output size; the header walk
 * of tarballs.nim:61-124 runs for all images at once: every 512-byte block is read as if it were a header, the
 * blocks reachable from an image's first block -- its headers -- are found by pointer doubling, and one wave per
 * header parses it and checks it (csrc/zh_tar_open_batch.hip).  The host parses no header byte.
 * More than 2^32 - 2 blocks of 512 bytes in one call (2 TiB of uncompressed images): ZH_ERR_ARGUMENT. */
int zh_tar_open_batch(zh_ctx *ctx, const void *const *images, const size_t *lens, size_t n_tar,
                      zh_tar_reader **readers, int32_t *statuses);

/* Tarball.open(stream, tarballFormat) of the v1 API -- tarballs_v1.nim:66-157 openStreamImpl -- for n_tar images per
 * call.  Not zh_tar_open_batch under another name: there is no end of archive, no long name, no symlink, no
 * unsupported type and no path check here (that is extractAll's, :294-309, and stays with the caller).
 * formats[t]: the caller's TarballFormat for image t; formats == NULL: all ZH_TF_DETECT.  statuses[t] is the outcome
 * of openStreamImpl on image t alone, the first check that fails:
 *   ZH_TF_DETECT (:80-88): byte 0 is 0x1F and byte 1 is 0x8B: gzip; byte 0 is 0x1F otherwise: ZH_ERR_TAR_FORMAT; else
 *     uncompressed;
 *   gzip (:94): the status zh_uncompress_batch(.., ZH_DF_GZIP, ..) gives the same bytes -- uncompress(data, dfGzip)
 *     with its CRC-32 and ISIZE checks, not trustSize;
 *   then, at pos (0 at first) while pos < len (:99):
 *     1. pos + 512 > len: ZH_ERR_TAR_EOF (:100);
 *     2. byte 0 of the name field is NUL: pos += 512 and on (:109-110) -- no other field of that header is read;
 *     3. the size, bytes 124..134, by strutils.parseOctInt: ZH_ERR_TAR_OPEN (:118);
 *     4. the mtime, bytes 136..146, likewise: ZH_ERR_TAR_OPEN (:124);
 *     5. the mode, bytes 100..105, likewise: ZH_ERR_TAR_OPEN_MODE (:131);
 *     6. pos + 512 + size > len: ZH_ERR_TAR_EOF (:139); contents that end the image without padding are accepted;
 *     7. typeflag '0' or NUL: contents[key] = a file; '5': = a directory; any other byte: nothing (:142-154);
 *     8. pos += 512 + (size + 511) & ~511 (:157).
 *   parseOctInt(s): an optional 0o / 0O when at least one byte follows it, then digits 0-7 and '_' (skipped); an
 *   error unless that is all of s and a digit was among them -- so a space or NUL inside the slice, an 8, or no digit.
 *   key = (prefix / name).toUnixPath(): name and prefix end at their first NUL or fill their 100 / 155 bytes; the
 *   prefix counts only when bytes 257..262 equal "ustar\0", the NUL included (GNU's "ustar  \0": no prefix); `/` is
 *   std/os's join (an empty prefix: the name alone; one '/' at a seam of two); toUnixPath turns every \ into /.
 *   contents[key] = entry replaces the value of an earlier equal key and keeps that key's place.
 * readers[t]: an ordinary reader -- zh_tar_num_entries / zh_tar_entry_at / zh_tar_data / zh_tar_close --, NULL when
 * statuses[t] != 0; a bad image never changes the others.  Its entries are the table's keys in the table's order:
 * path = the key; linkname_len = 0; a file: typeflag '0' (for '0' and NUL), mode = the six-byte octal, mtime, and
 * offset / size of the contents inside zh_tar_data(); a directory: typeflag '5' and every other field 0 whatever its
 * header says (TarballEntry(kind: ekDirectory), :150-154).  initTime(mtime, 0) and parseFilePermissions(mode) stay
 * with the caller.
 * Differences from the reference: it leaves a half-filled table behind its exception, the library returns no reader;
 * and where it raises a Defect, not a ZippyError, by indexing past the string -- ZH_TF_DETECT on an image of 0 bytes, or
 * of 1 byte that is 0x1F -- the library answers ZH_ERR_TAR_FORMAT.
 * The return value is a call-level error only: NULL arrays, an image that is NULL with a non-zero length, a format
 * outside 0..2 (ZH_ERR_ARGUMENT), allocation, device.  A plain image is borrowed until its reader is closed; the
 * uncompressed image of a gzip one is owned by its reader.  ctx is required; n_tar == 0 launches nothing.
 * Every gzip image of the call is decoded by one uncompress plan; the loop runs for all images at once: every
 * 512-byte block is read as if the loop stood on it, the blocks it does stand on are found by pointer doubling, and
 * one wave per named header parses it and checks it (csrc/zh_tar_read_batch.hip).  The host parses no header byte.
 * More than 2^32 - 2 blocks of 512 bytes in one call (2 TiB of uncompressed images): ZH_ERR_ARGUMENT. */
enum { ZH_TF_DETECT = 0, ZH_TF_UNCOMPRESSED = 1, ZH_TF_GZIP = 2 }; /* TarballFormat, tarballs_v1.nim:18-19 */
int zh_tar_read_batch(zh_ctx *ctx, const void *const *images, const size_t *lens, const int32_t *formats,
                      size_t n_tar, zh_tar_reader **readers, int32_t *statuses);

/* Writing tarballs: writeTarball(tarball, path) -- tarballs_v1.nim:203-270 -- for n_tar in-memory
 * tarballs at once, without the file write.  The host lays the images out and sends every entry's
 * contents straight to its place in HBM; one kernel writes the 512-byte ustar headers, the zero
 * padding and the 1024-byte trailers; for ZH_DF_GZIP the images are then compressed as one batch
 * (compress(image, level, dfGzip), tarballs_v1.nim:269, FNAME as zh_set_gzip_fname_len says). */
typedef struct zh_tar_new_entry { /* one TarballEntry of Tarball.contents (tarballs_v1.nim:8-15) */
  const char *path;               /* the table key; '/' is the only separator (std/os splitPath on POSIX) */
  size_t path_len;
  const void *contents;           /* may be NULL when len == 0 */
  size_t len;
  char kind;                      /* '0' (ekNormalFile) or '5' (ekDirectory); a directory's contents are written too */
  int64_t mtime;                  /* lastModified.toUnix() */
} zh_tar_new_entry;
enum { ZH_TAR_PLAIN = -1 };       /* data_format: the .tar image itself */
/* Tarball t is entries[first[t] .. first[t+1]) in insertion order (first has n_tar + 1 elements, non-decreasing).
 * data_format: ZH_TAR_PLAIN (.tar) or ZH_DF_GZIP (.tar.gz / .taz / .tgz); anything else returns
 * ZH_ERR_INVALID_FORMAT.  level: -2..9 as in zh_compress (ZH_DEFAULT_COMPRESSION is the drop-in value); ignored for
 * ZH_TAR_PLAIN.  dsts[t] is library-allocated (zh_free), NULL for a tarball that failed.
 * The return value is a call-level error: NULL pointers (also an entry's path or contents that is NULL with a
 * non-zero length), bad first[], level or format, allocation, device.  Everything about a tarball's own entries
 * is statuses[t]; a bad tarball never changes the bytes of the others:
 *  - ZH_ERR_TAR_EMPTY: no entries;
 *  - entry by entry in insertion order, the first failure wins; within one entry the checks run in this order:
 *    ZH_ERR_TAR_PATH (splitPath head >= 155 bytes), ZH_ERR_TAR_NAME (tail >= 100 bytes), then ZH_ERR_ARGUMENT
 *    for what the reference has no answer to or would write a broken header for:
 *      kind other than '0' / '5';
 *      len >= 8^11 or mtime outside [0, 8^11) (toOct(x, 11) would silently drop digits, and a negative
 *        time's unsigned conversion depends on the Nim version);
 *      a path equal to an earlier entry's of the same tarball (a table key cannot repeat).
 * Header bytes: name = tail, mode "000777 \0" (permissions are not written, as in the reference), uid / gid 0,
 * size and mtime in 11 octal digits, checksum, kind, "ustar\0" "00", devmajor / devminor 0, prefix = head;
 * contents zero-padded to 512 bytes; the image ends with 1024 zero bytes (tarballs_v1.nim:229-261). */
int zh_tar_create_batch(zh_ctx *ctx, const zh_tar_new_entry *entries, const size_t *first, size_t n_tar,
                        int data_format, int level, void **dsts, size_t *dst_lens, int32_t *statuses);

/* Writing zip archives: writeZipArchive(archive, path) -- ziparchives_v1.nim:371-486 -- for n_zip in-memory
 * archives at once, without the file write.  Every non-empty entry goes through ONE compress plan (deflate + its
 * CRC-32); the host lays the archives out from the compressed lengths, and one kernel writes every byte of every
 * image: local headers, the compressed streams gathered from the plan's slots, the central directories, the EOCDs. */
typedef struct zh_zip_new_entry { /* one (path, ArchiveEntry) of ZipArchive.contents (ziparchives_v1.nim:12-21) */
  const char *path;               /* the table key, bytes as given */
  size_t path_len;
  const void *contents;           /* may be NULL when len == 0 */
  size_t len;
  int is_directory;               /* ekDirectory: external attributes 0x10, else 0x20 (zh_zip_create_batch: not read) */
  uint16_t dos_time, dos_date;    /* toMsDos(lastModified) (:356-369), from the caller: the call stays pure */
                                  /* (zh_zip_create_batch: msdos(getTime()), the same pair for a whole archive) */
} zh_zip_new_entry;
/* Archive t is entries[first[t] .. first[t+1]) in insertion order (first has n_zip + 1 elements, non-decreasing).
 * level: -2..9 (ZH_DEFAULT_COMPRESSION gives the reference's bytes; other levels and contract mode give valid
 * archives with other deflate streams), else ZH_ERR_INVALID_LEVEL.  dsts[t] is library-allocated (zh_free), NULL for
 * an archive that failed.  The return value is a call-level error: NULL pointers (also an entry's path or contents
 * that is NULL with a non-zero length), bad first[] or level, allocation, device.  Everything about an archive's own
 * entries is statuses[t]; a bad archive never changes the bytes of the others.  The checks run step by step; within
 * a step, entry by entry in insertion order, and the first failure wins:
 *  1. ZH_ERR_ZIP_EMPTY: no entries (:375-376);
 *  2. ZH_ERR_ZIP_TOO_LARGE: more than 65535 entries, a path longer than 65535 bytes, or len >= 2^32 (the reference
 *     would truncate the value silently);
 *  3. ZH_ERR_ARGUMENT: contents that are not empty under method 0 (a path that is empty or ends in '/'; the
 *     reference would write deflate bytes under method 0);
 *  4. ZH_ERR_ZIP_DUPLICATE: a path equal to an earlier entry's of the same archive (a table key cannot repeat);
 *  5. after compression, ZH_ERR_ZIP_TOO_LARGE: a compressed length, a local header's offset, or the central
 *     directory's size or offset >= 2^32 (ZH_ZIP32_LIMIT, read at each call, lowers this limit: a test aid).
 * Paths are written as given: zh_zip_create's ZH_ERR_ZIP_NAME checks do not apply (v1 writes empty and absolute
 * paths).  Bytes (all little-endian, no zip64 records, :379-479):
 *  - each entry in insertion order: local header 50 4b 03 04, version 20, flags 0x0800, method, dos_time, dos_date,
 *    crc32(contents), compressed length, length, path length, extra length 0, the path, the compressed stream.
 *    Method 0 when the contents are empty or splitFile(path).name is empty (the path is empty or ends in '/'): no
 *    data, CRC 0, both lengths 0; else method 8 and compress(contents, level, dfDeflate);
 *  - the central directory in the same order: 50 4b 01 02, made-by 63, version 20, flags 0x0800, method, time, date,
 *    CRC, both lengths, path length, extra / comment / disk / internal attributes 0, external attributes
 *    10 00 00 00 (directory) or 20 00 00 00, the local header's offset, the path;
 *  - the end of central directory record: 50 4b 05 06, 0, 0, the entry count twice, the directory's size and offset,
 *    comment length 0. */
int zh_zip_write_batch(zh_ctx *ctx, const zh_zip_new_entry *entries, const size_t *first, size_t n_zip,
                       int level, void **dsts, size_t *dst_lens, int32_t *statuses);

/* createZipArchive(entries: OrderedTable[string, string]) -- ziparchives.nim:455-634 -- for n_zip in-memory archives
 * at once: zh_zip_create's archives through zh_zip_write_batch's pipeline (one compress plan with CRC-32 over every
 * non-empty entry of the call, the layout on the host from the compressed lengths, one kernel that writes every
 * byte of every image, one download).  The shape, the ownership and the split of the errors are those of
 * zh_zip_write_batch: archive t is entries[first[t] .. first[t+1]) in insertion order; dsts[t] is library-allocated
 * (zh_free), NULL for an archive that failed; the return value is a call-level error (NULL pointers, also an entry's
 * path or contents that is NULL with a non-zero length; bad first[]; a level outside -2..9, ZH_ERR_INVALID_LEVEL,
 * checked before the table; more than 2^32 - 2 entries or archives in the call, ZH_ERR_ARGUMENT; allocation;
 * device); everything about an archive's own entries is statuses[t], and a bad archive never changes the bytes of
 * the others.  n_zip == 0 returns ZH_OK.
 * Entries: zh_zip_new_entry, of which `is_directory` is NOT read (createZipArchive writes external attributes 0).
 * dos_time / dos_date are written per entry; the reference stamps every entry of a call with one msdos(getTime())
 * (:475-493), so a caller gets the reference's bytes by giving all entries of an archive the same pair.
 * level: ZH_BEST_SPEED gives the reference's bytes (:530); other levels and contract mode (zh_set_l1_parse(ctx, 1))
 * give valid archives with other deflate streams.
 * Statuses: entry by entry in PROCESSING order, which is last to first (the reference pops keys off the table's end,
 * :503-505), the first failure wins; within one entry, in zh_zip_create's order:
 *  1. ZH_ERR_ZIP_NAME: an empty path;
 *  2. ZH_ERR_ZIP_NAME: a path that starts with '/';
 *  3. ZH_ERR_ZIP_NAME: a path longer than 65535 bytes;
 *  4. ZH_ERR_ZIP_DUPLICATE: a path equal to that of an entry checked before it (a table key cannot repeat);
 * after compression, the first entry's compress status (same order) that is not ZH_OK.
 * An archive without entries is valid: its three end records, 98 bytes.  There are no 32-bit limits: every length
 * and offset is 64-bit (an entry of 4 GiB and more is legal), the entry count too; ZH_ZIP32_LIMIT is not read.
 * Bytes (all little-endian, :541-624):
 *  - each entry, LAST TO FIRST: local header 50 4b 03 04, version 45, flags 0x0800, method, dos_time, dos_date,
 *    crc32(contents), ff ff ff ff twice, path length, extra length 20; the path; the zip64 extra (id 1, size 16,
 *    u64 length, u64 compressed length); the stream.  Method 0, no stream and CRC 0 when the contents are empty,
 *    else method 8 and compress(contents, level, dfDeflate);
 *  - the central directory in the same order: 50 4b 01 02, made-by 45, needed 45, flags 0x0800, method, time, date,
 *    CRC, ff ff ff ff twice, path length, extra length 28, comment length / disk / internal / external attributes 0,
 *    offset ff ff ff ff; the path; the zip64 extra (id 1, size 24, length, compressed length, local header offset);
 *  - the zip64 end of central directory record (56 bytes: 50 4b 06 06, 44, 45, 45, disks 0 0, the entry count twice,
 *    the directory's size and offset), its locator (20 bytes: 50 4b 06 07, 0, the zip64 end record's offset, 1) and
 *    the end of central directory record (22 bytes: 50 4b 05 06, 0, 0, counts, size and offset ff-filled, 0). */
int zh_zip_create_batch(zh_ctx *ctx, const zh_zip_new_entry *entries, const size_t *first, size_t n_zip,
                        int level, void **dsts, size_t *dst_lens, int32_t *statuses);

/* ------------------------------------------------------------------ *
 * Introspection for parity tests (not part of the drop-in surface).   *
 * ------------------------------------------------------------------ */
/* Level-1 parse of one buffer as the u16 token stream of SURVEY.md 8a row a4
 * (snappy.nim:33-64 format), block by block, fragment by fragment: lets tests
 * compare the device matcher with the oracle token-for-token.  tokens is
 * library-allocated (zh_free).  At level 1 it follows zh_set_l1_parse / ZH_L1_PARSE as compress does: in contract
 * mode the tokens are the parallel parse's (zh_l1p_match.hip), which the tests hold against the rule of
 * tests/l1p_model.py token for token (check_l1p_tokens); with the switch off nothing changes. */
int zh_debug_tokens(zh_ctx *ctx, const void *src, size_t len, int level, uint16_t **tokens,
                    size_t *num_tokens);
/* Debug hook: ONE prefix code from a histogram of num_freq <= 288 symbols (deflate.nim:13-151 huffmanCodes:
 * min_codes as the reference's minCodes, limit <= 15 bits).  contract 0: the replay of the reference (its heap
 * order, its length limiting) -- the tests hold it against the oracle symbol for symbol; 1: contract mode's
 * builder (zh_set_l1_parse(ctx, 1)) -- other tie-breaks; optimal unless the length limit binds (then repaired the
 * way zlib / miniz do: valid, not always the minimum).  codes (bit-reversed, as they
 * go into the stream) and lens hold num_freq + 2 entries; *num_codes is the reference's numCodes (min_codes <=
 * num_freq, as in every call of the reference's: anything else is ZH_ERR_ARGUMENT). */
int zh_debug_huffman(zh_ctx *ctx, const uint32_t *freq, int num_freq, int min_codes, int limit, int contract,
                     uint16_t *codes, uint8_t *lens, int *num_codes);
/* Large streams are decoded by many workgroups each (segment-wise) when the chain of their segments holds, by one
 * workgroup otherwise -- same bytes and statuses either way, so only a count can tell the two apart: since the
 * context was made, *cut = streams that uncompress runs cut into segments, *held = those of them whose chain held.
 * Counted on the device by EVERY run of a segmented plan -- a sizing (count-only) pass and a re-run of the same plan
 * count again --, so compare differences around the runs of interest.  A stream that is damaged, or has fewer than
 * four block starts and sub-starts, legitimately does not hold. */
int zh_debug_segment_stats(zh_ctx *ctx, uint64_t *cut, uint64_t *held);

#ifdef __cplusplus
}
#endif
#endif
