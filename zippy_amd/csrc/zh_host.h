// Host side of the C ABI, shared declarations (not installed: include/zippy_hip.h is the public header).
// The host side lives in eighteen files -- zh_context.hip (contexts, the device block cache, bounds),
// zh_plan_compress.hip / zh_plan_uncompress.hip (device-resident plans: descriptors and scratch),
// zh_plan_run.hip (kernel sequencing -- run_compress, run_uncompress with run_segmented, run_ranges; work beside a run
// on the context's second stream: SideLane --, switches, results), zh_plan_pack.hip (a plan's streams back to back for the
// wire), zh_host_batch.hip (host-buffer batches: staging, pipelined groups, sharding over contexts),
// zh_host_calls.hip (single-buffer calls, the block-parallel form, checksums, debug hooks), zh_ranges.hip (byte-range
// reads from block-indexed streams: geometry, host call and its two kernels), zh_seek.hip (seek indexes for foreign
// streams: build, range reads and their kernels), zh_resume.hip (resumable uncompress: the host call and the resuming
// form of the wave-pair kernel), zh_stream.hip (streaming compress: the host call and the two kernels that splice a
// piece's stream behind the bits pending from the call before), the batch writers
// zh_zip_write.hip / zh_tar_create.hip and the batch readers zh_tar_open_batch.hip / zh_tar_read_batch.hip /
// zh_zip_open_batch.hip / zh_zip_read_batch.hip (whose kernels sit next to their host code; zh_walk.h holds the walk
// all four share, zh_scan.h the signature scan of zh_zip_read_batch.hip and zh_bgzf.hip with its host driver,
// zh_tar_dev.h and zh_zip_dev.h what the two of a format share, zh_gather.h the unaligned copy), and zh_bgzf.hip (BGZF
// written, read, indexed and read by range; zh_range_host.h holds the host arithmetic its range read shares with
// zh_ranges.hip).
// No compute happens on the host.  This header also holds what those files build their device memory with: DevMem /
// DevBuf (owners that free through the context's cache) and Arena (the device arrays of a plan or call, each declared once).
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "zh_common.h"
#include "zh_kprof.h"
#include "zh_tables.h"

#define ZH_INTERNAL __attribute__((visibility("hidden")))

// ---- kernel launchers (defined next to their kernels) ----
extern "C" {
const void* zh_checksum_tables(int device);
void zh_launch_checksum_pieces(hipStream_t, const void* tabs, const uint8_t* d_data,
                               const ZhPieceDesc* pieces, uint32_t npieces, const uint64_t* dyn_len,
                               int want_crc, int want_adler, uint32_t* out_crc, uint32_t* out_adler,
                               uint32_t* out_len);
void zh_launch_checksum_combine(hipStream_t, const void* tabs, const ZhBufDesc* bufs, uint32_t nbufs,
                                const uint32_t* piece_crc, const uint32_t* piece_adler,
                                const uint32_t* piece_len, int want_crc, int want_adler,
                                uint32_t* buf_crc, uint32_t* buf_adler);
void zh_launch_unwrap(hipStream_t, const uint8_t* d_src, ZhInflateArgs a);
void zh_launch_inflate(hipStream_t, const uint8_t* d_src, uint8_t* d_dst, ZhInflateArgs a);
void zh_launch_seek_inflate(hipStream_t, const uint8_t* d_src, uint8_t* d_dst, ZhInflateArgs a, ZhSeekStop x);
void zh_launch_resume_inflate(hipStream_t, const uint8_t* d_src, uint8_t* d_dst, ZhInflateArgs a, ZhResume r);
void zh_launch_verify(hipStream_t, ZhInflateArgs a, const uint32_t* buf_crc, const uint32_t* buf_adler);
void zh_launch_inflate_tokens(hipStream_t, const uint8_t* d_src, ZhInflateArgs a, uint32_t* tok_pool,
                              const uint64_t* tok_off, const uint64_t* tok_cap, const ZhRecArgs* rec);
void zh_launch_inflate_write(hipStream_t, const uint8_t* d_src, uint8_t* d_dst, ZhInflateArgs a,
                             const uint32_t* tok_pool, const uint64_t* tok_off);
void zh_launch_inflate_count(hipStream_t, const uint8_t* d_src, ZhInflateArgs a);
void zh_launch_inflate_spec(hipStream_t, const uint8_t* d_src, ZhInflateArgs a, ZhRecArgs rec);
void zh_launch_segments_reduce(hipStream_t, ZhInflateArgs seg, ZhInflateArgs whole);
void zh_launch_seg_find(hipStream_t, const uint8_t* d_src, ZhInflateArgs a, ZhSegArgs g);
void zh_launch_seg_fake_start(hipStream_t, ZhSegArgs g, uint64_t bit);
void zh_launch_seg_check(hipStream_t, const uint8_t* d_src, ZhInflateArgs a, ZhSegArgs g);
void zh_launch_seg_tokens(hipStream_t, const uint8_t* d_src, ZhInflateArgs a, uint32_t* tok_pool, ZhSegArgs g, int phase);
void zh_launch_seg_decide(hipStream_t, ZhInflateArgs a, ZhSegArgs g, int rerun);
void zh_launch_seg_chain(hipStream_t, ZhInflateArgs a, ZhSegArgs g, int rerun);
void zh_launch_seg_repair(hipStream_t, ZhInflateArgs a, ZhSegArgs g);
void zh_launch_seg_stats(hipStream_t, ZhSegArgs g, uint64_t* stats);
void zh_launch_seg_write(hipStream_t, const uint8_t* d_src, ZhInflateArgs a, const uint32_t* tok_pool, ZhSegArgs g);
void zh_launch_seg_windows(hipStream_t, ZhInflateArgs a, ZhSegArgs g);
void zh_launch_seg_finish(hipStream_t, uint8_t* d_dst, ZhInflateArgs a, ZhSegArgs g);
ZhL1Launch zh_l1_match_prepare(hipStream_t, uint32_t nfrags, uint32_t* next_frag, uint32_t* cost, uint32_t* order,
                               uint32_t* hist, int use_order, int side_ok);
void zh_launch_l1_match(hipStream_t, const uint8_t* d_src, ZhCompressArgs a, int huffman_only,
                        uint16_t* table_pool, uint32_t* next_frag, uint32_t* cost, ZhL1Launch l, int lds_part);
uint32_t zh_l1_table_slots(void);
void zh_launch_l1p_match(hipStream_t, const uint8_t* d_src, ZhCompressArgs a, uint16_t* link_pool,
                         uint32_t* next_frag);
uint32_t zh_l1p_slots(void);
void zh_launch_chain_prev(hipStream_t, const uint8_t* d_src, ZhCompressArgs a, uint32_t* head_scratch,
                          uint64_t* prevw, uint32_t* lists, int links_serial, int good);
uint32_t zh_chain_prev_slice(void);
int zh_chain_lds_order_ok(int device, hipStream_t stream);
void zh_launch_chain_search(hipStream_t, const uint8_t* d_src, ZhCompressArgs a, int good, int nice,
                            int max_chain, const uint64_t* prevw, uint32_t* best, int links_serial);
void zh_launch_chain_select(hipStream_t, const uint8_t* d_src, ZhCompressArgs a, int good, int nice,
                            int max_chain, const uint64_t* prevw, uint32_t* best, int links_serial);
void zh_launch_frag_stats(hipStream_t, const uint8_t* d_src, ZhCompressArgs a);
void zh_launch_huffman(hipStream_t, ZhCompressArgs a, int contract);
void zh_launch_huffman_probe(hipStream_t, const uint32_t* freq, int num_freq, int min_codes, int limit, int contract,
                             uint16_t* codes, uint8_t* lens, int* n_out);
void zh_launch_layout(hipStream_t, uint8_t* d_dst, ZhCompressArgs a, const uint32_t* buf_crc,
                      const uint32_t* buf_adler, int with_trailer);
void zh_launch_trailer(hipStream_t, uint8_t* d_dst, ZhCompressArgs a, const uint32_t* buf_crc, const uint32_t* buf_adler);
void zh_launch_emit(hipStream_t, const uint8_t* d_src, uint8_t* d_dst, ZhCompressArgs a, int cover_in);
}

// ---- byte-range reads from block-indexed streams (zh_ranges.hip) ----
// One piece of at most kClipChunk bytes of an edge block's (zh_ranges.hip) or edge member's (zh_bgzf.hip) bytes on its
// way from the scratch into a range's slot.
constexpr uint32_t kClipChunk = 16384;  // bytes of a clip a workgroup moves
struct ZhClipDesc {
  uint64_t src;  // byte offset in the scratch
  uint64_t dst;  // byte offset in d_dst
  uint32_t len, pad;
};
// Device arrays of a ranges plan.  The blocks' arrays hold the blocks decoded in place first, the edge blocks (decoded
// into scratch) behind them: a group of ranges is a launch over a stretch of either part.
struct ZhRangesArgs {
  const ZhBufDesc* bufs;        // [nblocks] src_off / src_len: the compressed bytes; dst_off / dst_cap: slot and promised size
  const uint64_t* start_bit;    // [nblocks] the block's first bit, counted from src_off
  uint64_t* blk_len;            // [nblocks] bytes the block's decoder made
  int32_t* blk_status;          // [nblocks]
  const uint32_t* first_block;  // [nranges + 1] range r's blocks are order[first_block[r] .. first_block[r + 1]) ...
  const uint32_t* order;        //   ... positions in the blocks' arrays, in index order
  const int32_t* fixed_status;  // [nranges] decided when the plan was made (ZH_OK: by the blocks)
  const uint64_t* clip_len;     // [nranges] the range's length clipped at the stream's end
  const ZhClipDesc* clips;
  uint64_t* out_len;            // [nranges]
  int32_t* status;              // [nranges]
  uint32_t nranges;
};
extern "C" {
void zh_launch_range_clip(hipStream_t, const uint8_t* d_scratch, uint8_t* d_dst, const ZhClipDesc* clips, uint32_t nclips);
void zh_launch_ranges_reduce(hipStream_t, ZhRangesArgs a);
}
// internal.nim:177-189 configurationTable (good, nice, chain); `lazy` is unused by the reference
static const int kChainConfig[10][3] = {{0, 0, 0},     {4, 8, 4},      {4, 16, 8},    {4, 32, 32},
                                        {4, 16, 16},   {8, 32, 32},    {8, 128, 128}, {8, 256, 256},
                                        {32, 258, 1024}, {32, 258, 4096}};

struct zh_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int fname_len = -1;
  int inflate_mode = -1;  // -1: ZH_INFLATE or the default (split), 0 split, 1 serial
  int l1_parse = -1;      // -1: ZH_L1_PARSE or the default (exact), 0 exact (the reference's parse), 1 parallel
  // chain levels: THIS device failed zh_create's probe of the LDS atomic lane order (zh_chain_match.hip): its links
  // come from the in-order kernels
  bool chain_links_serial = false;
  std::string last_error;
  uint64_t* d_seg_stats = nullptr;  // zh_debug_segment_stats: two device counters (streams cut into segments / whose chain held)
  const void* cktabs = nullptr;
  std::mt19937 rng{std::random_device{}()};
  // host-buffer calls: two pinned staging chunks between the caller's pageable memory and HBM
  // (allocated on the first such call)
  uint8_t* pin[2] = {nullptr, nullptr};
  hipEvent_t pin_ev[2] = {nullptr, nullptr};
  bool pin_busy[2] = {false, false};
  hipStream_t copy_stream = nullptr;  // transfers of a pipelined batch, next to `stream`'s kernels
  // a compress run's checksum kernels beside its code builder (zh_plan_run.hip): forked off `stream` behind the match
  // finder, joined in front of the layout; the events are the context's (runs of one context follow each other)
  hipStream_t aux_stream = nullptr;
  hipEvent_t aux_fork = nullptr, aux_join = nullptr;
  uint64_t pipe_min = 0, pipe_group = 0;  // zh_set_host_pipeline (0: ZH_PIPE_MIN / ZH_PIPE_GROUP / default)
  // device memory the context has freed, kept for its next call (ctx_malloc / ctx_free)
  struct DevBlock {
    void* p;
    size_t size;
    bool used;
    uint64_t stamp;
  };
  std::vector<DevBlock> dev_blocks;
  // zh_debug_range_stats: the last ranges call / plan run (bytes over the link, blocks decoded in place / via scratch)
  uint64_t rg_uploaded = 0, rg_in_place = 0, rg_via_scratch = 0;
  // zh_debug_gzip_stats: the last zh_gzip_read_batch (candidates, input bytes its speculative pass consumed, frontier rounds)
  uint64_t gz_candidates = 0, gz_spec_bytes = 0, gz_rounds = 0;
  size_t dev_cached = 0, dev_cache_max = 0;
  uint64_t dev_stamp = 0;
  bool dev_poison = false;
};

// (zh_context.hip)
ZH_INTERNAL hipError_t ctx_malloc(zh_ctx* ctx, void** out, size_t bytes);
ZH_INTERNAL void ctx_free(zh_ctx* ctx, void* p);

#define ZH_HIP(ctx, call)                                                            \
  do {                                                                               \
    hipError_t e_ = (call);                                                          \
    if (e_ != hipSuccess) {                                                          \
      (ctx)->last_error = std::string(#call) + ": " + hipGetErrorString(e_);         \
      return ZH_ERR_DEVICE;                                                          \
    }                                                                                \
  } while (0)

static inline size_t container_overhead(int fmt) {
  return fmt == ZH_DF_GZIP ? 10 + 26 + 8 : fmt == ZH_DF_ZLIB ? 6 : 0;
}
static inline size_t typical_cap(size_t len, int fmt) {
  size_t nblocks = (len + ZH_BLOCK_SIZE - 1) / ZH_BLOCK_SIZE;
  if (!nblocks) nblocks = 1;
  return len + len / 8 + 1024 * nblocks + 5 * (len / ZH_STORED_MAX + 1) + container_overhead(fmt) + 64;
}

// ---------------------------------------------------------------------------
// plans
// ---------------------------------------------------------------------------
// Device memory from the context's cache that goes back to it with its owner (ctx_malloc / ctx_free)
template <class T>
struct DevMem {
  T* p = nullptr;
  zh_ctx* ctx = nullptr;
  DevMem() = default;
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  void release() {
    if (p) ctx_free(ctx, p);
    p = nullptr;
  }
  ~DevMem() { release(); }
};
using DevBuf = DevMem<uint8_t>;
template <class T>
static inline hipError_t dev_alloc(zh_ctx* ctx, DevMem<T>& b, size_t bytes) {
  void* q = nullptr;
  const hipError_t e = ctx_malloc(ctx, &q, bytes);
  b.ctx = ctx;
  b.p = e == hipSuccess ? static_cast<T*>(q) : nullptr;
  return e;
}

// The device arrays of a plan or a call in one allocation, each declared once: add() takes the pointer to set, the
// number of elements (their size is the pointee's) and, for an array that is uploaded, its host source.  Every array
// starts at the next multiple of 256, in the order of the add() calls; an empty one still has its place, and its
// pointer is not null.  alloc() takes `size` bytes from the context's cache, bind() sets every pointer, upload() sends
// every source.  The pointers registered stay where they are until bind(), the sources until upload() has been waited for.
struct Arena {
  struct Slot {
    void* target;
    void (*set)(void* target, uint8_t* at);
    size_t off, bytes;
    const void* src;
  };
  std::vector<Slot> slots;
  size_t size = 0;
  uint8_t* base = nullptr;
  template <class T>
  void add(T*& ptr, size_t count, const typename std::remove_const<T>::type* src = nullptr) {
    const size_t bytes = count * sizeof(T);
    slots.push_back(Slot{(void*)&ptr, [](void* target, uint8_t* at) { *static_cast<T**>(target) = reinterpret_cast<T*>(at); },
                         pad(bytes), bytes, src});
  }
  // bytes nothing points at (a tail behind the last array for kernels that read whole words or vectors) -> their offset
  size_t pad(size_t bytes) {
    const size_t off = (size + 255) & ~(size_t)255;
    size = off + bytes;
    return off;
  }
  hipError_t alloc(zh_ctx* ctx, DevBuf& mem, size_t extra = 0) {
    const hipError_t e = dev_alloc(ctx, mem, size + extra);
    base = mem.p;
    return e;
  }
  void bind() const {
    for (const Slot& s : slots) s.set(s.target, base + s.off);
  }
  hipError_t upload(hipStream_t stream) const {  // (the first error ends it)
    for (const Slot& s : slots) {
      if (!s.src || !s.bytes) continue;
      const hipError_t e = hipMemcpyAsync(base + s.off, s.src, s.bytes, hipMemcpyHostToDevice, stream);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  // ... or copies them into a host image of the arena's first bytes, which the caller uploads in one piece
  void gather(uint8_t* image) const {
    for (const Slot& s : slots)
      if (s.src && s.bytes) memcpy(image + s.off, s.src, s.bytes);
  }
  // the bound array `dev` in a host copy `image` of the arena's first bytes (a download of the caller's)
  template <class T>
  const T* host(const void* image, const T* dev) const {
    return reinterpret_cast<const T*>(static_cast<const uint8_t*>(image) + (reinterpret_cast<const uint8_t*>(dev) - base));
  }
  // the array declared for `ptr`, all zero (its size is the declaration's)
  template <class T>
  hipError_t clear(T*& ptr, hipStream_t stream) const {
    for (const Slot& s : slots)
      if (s.target == (void*)&ptr) return hipMemsetAsync(base + s.off, 0, s.bytes, stream);
    return hipErrorInvalidValue;
  }
};

// Device-resident plans keep their per-position scratch -- the chain levels' links and best matches (12 bytes a
// position), the split decoder's token records (4 bytes an output byte) -- for at most this many bytes at a time;
// a batch that needs more runs those kernels over ranges of its blocks / streams, one range after the other
// through the same scratch (same bytes out).  ZH_SCRATCH_MB (default 32768: BASELINE's 4096 x 1 MiB batch decodes
// as one group -- its records take 16.8 GiB, and two launches of 2048 streams measured 12 % slower than one of
// 4096 --; the tests force it low).
static inline uint64_t scratch_budget() {
  const char* e = getenv("ZH_SCRATCH_MB");
  const uint64_t mb = e ? strtoull(e, nullptr, 10) : 32768ull;
  return (mb ? mb : 1ull) << 20;
}

// (zh_ranges.hip)
struct ZhRangesPlan {
  ZhRangesArgs a{};
  DevBuf arena, scratch;
  uint32_t n_in_place = 0, n_scratch = 0;
  // the groups of ranges that share the scratch in turn: stretches of the in-place blocks, the edge blocks and the clips
  struct Group {
    uint32_t ip0, nip, sc0, nsc, clip0, nclip;
  };
  std::vector<Group> groups;
};

struct ZhPlanRange {
  uint32_t b0, nb, f0, nf;
};
// The timing events of a profiled run on one stream and the names of the launches they were recorded in front of
// (prof_mark, zh_plan_kernel_times)
struct ProfLane {
  std::vector<const char*> names;
  std::vector<hipEvent_t> events;
};
struct zh_plan {
  zh_ctx* ctx = nullptr;
  bool is_compress = true;
  size_t n = 0;
  int level = 0, fmt = 0;
  DevBuf arena;
  ZhCompressArgs ca{};
  ZhInflateArgs ia{};
  ZhBufDesc* d_bufs = nullptr;
  ZhPieceDesc* d_pieces = nullptr;
  uint32_t npieces = 0;
  uint32_t *piece_crc = nullptr, *piece_adler = nullptr, *piece_len = nullptr;
  uint32_t *buf_crc = nullptr, *buf_adler = nullptr;
  // chain levels: `head` per block, previous-position links and best match per position (zh_chain_match.hip)
  uint32_t* head_scratch = nullptr;
  uint16_t* l1_tables = nullptr;  // BestSpeed: pool of per-wave hash tables (zh_l1_match.hip)
  void* l1_pool_own = nullptr;    // ... when it is an allocation of its own (ZH_L1_POOL: uncached / fine-grained memory)
  uint32_t* l1_counter = nullptr; // ... and the counter its waves draw fragments from
  // longest first (zh_l1_match.hip): a fragment's cycles in the last run, the order made of them, scratch; l1_runs: runs so far
  uint32_t *l1_cost = nullptr, *l1_order = nullptr, *l1_hist = nullptr;
  uint32_t l1_runs = 0;
  uint64_t* chain_prev = nullptr;
  uint32_t* chain_best = nullptr;
  // best[] is cleared when the plan is made and handed back cleared by every run's link kernels; a run that
  // did not get as far (a launch that failed between the scatter and the links) leaves it dirty, and the next
  // run clears it before anything reads it
  bool chain_best_dirty = false;
  // chain levels: the ranges of blocks (first block, blocks, first fragment, fragments) that share the scratch in turn
  std::vector<ZhPlanRange> chain_ranges;
  size_t chain_scratch_frags = 0;  // fragments the scratch holds (the largest range)
  // split inflate: the groups of streams (first, count) that share the token pool in turn
  std::vector<std::pair<uint32_t, uint32_t>> tok_groups;
  uint64_t dst_max_cap = 0;
  uint64_t* out_len = nullptr;
  int32_t* status = nullptr;
  uint64_t src_max_len = 0;      // uncompress plans: the longest source slot (zh_plan_unpack's grid)
  DevMem<uint64_t> unpack_lens;  // ... and the device-side lengths zh_plan_unpack leaves (allocated by its first call)
  // block index (zh_plan_block_index): host copies of the geometry
  std::vector<ZhBufDesc> h_bufs;
  uint32_t half_piece = 0;  // uncompress plans: the first checksum piece of buffer n / 2 (the batch as two halves, zh_plan_run)
  std::vector<ZhBlockDesc> h_blocks;
  // block-parallel decode (zh_plan_uncompress_indexed): `ia` describes the one stream, `seg` its blocks
  bool force_crc = false;  // CRC-32 of the uncompressed side whatever the container (ZIP entries)
  bool indexed = false;
  // split inflate (zh_inflate_split.hip): per-stream token buffers, allocated on the first run (tok_own) or the
  // caller's (pipelined groups share one: plan_lend_token_pool)
  uint32_t* tok_pool = nullptr;
  DevMem<uint32_t> tok_own;
  uint64_t tok_words = 0;
  const uint64_t *tok_off = nullptr, *tok_cap = nullptr;
  bool tok_failed = false;
  ZhInflateArgs seg{};
  DevBuf seg_arena;
  // an index build (zh_seek.hip): where the tokens kernel records its points (points null: an ordinary plan)
  ZhRecArgs rec{};
  // byte-range reads (zh_plan_uncompress_ranges): n ranges; nothing above describes such a plan but ctx, n, out_len, status
  std::unique_ptr<ZhRangesPlan> rg;
  // large streams decoded segment-wise (zh_inflate_seg.hip); the symbol and window buffers come
  // with the token pool
  bool segmented = false;
  // test aids read when the plan is made (not on the run path): ZH_SEG_FAKE_START (a stream bit, ~0: none), ZH_TRACE_SEG
  uint64_t sg_fake_start = ~0ull;
  bool sg_trace = false;
  int sg_repair_rounds = 1;  // zh_seg_repair_kernel: twice where there is a lot to go wrong (plan_segments)
  ZhSegArgs sg{};
  DevBuf sg_arena;
  DevMem<uint16_t> sg_sym;
  DevBuf sg_windows;
  DevMem<uint16_t> sg_winsym;
  uint64_t sg_sym_count = 0;
  // profiling
  bool profiling = false;
  bool trailer_late = false;  // compress: the checksum joins behind the emission (large batches; zh_plan_run.hip)
  // uncompress: batches of at least this many streams go as two halves on two streams (0: never; zh_plan_run.hip)
  uint32_t halves_min = 0;
  // the launches on the context's stream, and those beside them on its second stream (the checksum of a compress
  // run, the second half of an uncompress batch): reported behind the others
  ProfLane k_main, k_side;
};

// What can be said of a block index without decoding (zh_plan_uncompress_indexed, zh_plan_uncompress_ranges): at
// least one block, entry 0 at output byte 0, neither offset ever falling, every block's first bit inside the stream.
static inline bool block_index_sound(const zh_block_entry* index, size_t n_entries, uint64_t src_len) {
  if (n_entries < 2 || index[0].out_off != 0) return false;
  for (size_t k = 0; k + 1 < n_entries; k++)
    if (index[k + 1].out_off < index[k].out_off || index[k + 1].bit_off < index[k].bit_off ||
        index[k].bit_off >= src_len * 8)
      return false;
  return true;
}
// One deflate block as the "stream" of a decoder that stops behind one block (zh_inflate_kernel with start_bit)
static inline ZhBufDesc block_decoder_desc(uint64_t src_off, uint64_t src_len, uint64_t dst_off, uint64_t dst_cap) {
  ZhBufDesc b;
  memset(&b, 0, sizeof(b));
  b.src_off = src_off;
  b.src_len = src_len;
  b.dst_off = dst_off;
  b.dst_cap = dst_cap;
  return b;
}
// ... and the launch of such decoders: `whole` stripped of everything a whole stream has
static inline ZhInflateArgs block_decoder_args(const ZhBufDesc* bufs, const uint64_t* start_bit, uint32_t n,
                                               uint64_t* out_len, int32_t* status) {
  ZhInflateArgs g{};
  g.bufs = bufs;
  g.nbufs = n;
  g.start_bit = start_bit;
  g.single_block = 1;
  g.out_len = out_len;
  g.status = status;
  return g;
}

static inline bool valid_block_bytes(size_t bb) {
  return bb >= ZH_FRAG_SIZE && bb <= ZH_BLOCK_SIZE && bb % ZH_FRAG_SIZE == 0;
}

// (zh_plan_run.hip)
ZH_INTERNAL bool inflate_split_enabled(const zh_ctx* ctx);
ZH_INTERNAL bool l1_parallel(const zh_ctx* ctx);
ZH_INTERNAL int run_l1_match(zh_plan* p, const uint8_t* d_src, bool with_order);
ZH_INTERNAL bool plan_token_pool(zh_plan* p);
ZH_INTERNAL void plan_lend_token_pool(zh_plan* p, uint32_t* pool, uint64_t words);
static inline void plan_set_count_only(zh_plan* plan, int on) { plan->ia.count_only = on; }

// ---------------------------------------------------------------------------
// host-buffer API: device buffers of a call, plans that go away with their scope, phase timing
// ---------------------------------------------------------------------------
struct PlanGuard {
  zh_plan* p = nullptr;
  ~PlanGuard() { zh_plan_destroy(p); }
};

// ZH_TRACE=1: wall-clock of the host-buffer calls' phases on stderr (tuning aid; syncs the stream)
struct Trace {
  bool on = getenv("ZH_TRACE") != nullptr;
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void mark(zh_ctx* ctx, const char* what) {
    if (!on) return;
    (void)hipStreamSynchronize(ctx->stream);
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[zh] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
    t = now;
  }
};


// a batch call's three output arrays as they are before anything is handed out
static inline void clear_outputs(void** dsts, size_t* dst_lens, int32_t* statuses, size_t n) {
  for (size_t i = 0; i < n; i++) {
    dsts[i] = nullptr;
    dst_lens[i] = 0;
    statuses[i] = ZH_OK;
  }
}

// (zh_host_batch.hip) pack host buffers into one device allocation / results into fresh host buffers
ZH_INTERNAL int zhh_upload(zh_ctx* ctx, const void* const* srcs, const size_t* lens, size_t n, DevBuf& dev,
                           std::vector<uint64_t>& off, std::vector<uint64_t>& len64);
// host buffers -> dev at arbitrary byte offsets: srcs[i] (len64[i] bytes) lands at dev + off[i], off[] ascending;
// the whole range [0, total) goes over the link, so bytes between the slices hold stale staging contents afterwards
ZH_INTERNAL int zhh_upload_slices(zh_ctx* ctx, const void* const* srcs, const std::vector<uint64_t>& off,
                                  const std::vector<uint64_t>& len64, uint64_t total, uint8_t* dev);
ZH_INTERNAL int zhh_download(zh_ctx* ctx, const uint8_t* d_dst, size_t n, const std::vector<uint64_t>& doff,
                             const std::vector<uint64_t>& olen, const std::vector<char>& take, void** dsts,
                             size_t* dst_lens, int32_t* statuses);
// host byte spans packed into one device buffer, each at a 16-byte aligned offset off[k], in one upload
ZH_INTERNAL int zhh_upload_spans(zh_ctx* ctx, std::initializer_list<std::pair<const void*, size_t>> spans, DevBuf& dev,
                                 std::vector<uint64_t>& off);
// One compress plan over the device buffers d_src + soff[i] (slen[i] bytes each), run once more with every output
// slot at zh_compress_bound when a buffer did not fit its first slot (the first attempt's slots are freed before the
// second's are allocated).  On ZH_OK, dst holds the last attempt's slots and doff / clen / cst its results (crcs, if
// given: the CRC-32 of every buffer).  n == 0 does nothing.
ZH_INTERNAL int zhh_compress(zh_ctx* ctx, const uint8_t* d_src, const std::vector<uint64_t>& soff,
                             const std::vector<uint64_t>& slen, int level, int fmt, uint32_t* crcs, DevBuf& dst,
                             std::vector<uint64_t>& doff, std::vector<uint64_t>& clen, std::vector<int32_t>& cst);

// (zh_tar.hip) the readers zh_tar_open_batch builds from its kernels' records: an empty reader over `data` (owned: the
// reader's to release, or NULL for a borrowed image), then its entries in walk order
extern "C" {
ZH_INTERNAL zh_tar_reader* zh_tar_reader_new(void* owned, const void* data, size_t len);
ZH_INTERNAL int zh_tar_reader_add(zh_tar_reader* r, const char* path, size_t path_len, const char* linkname,
                                  size_t linkname_len, char typeflag, uint32_t mode, int64_t mtime, uint64_t offset,
                                  uint64_t size);
}

// ---- the batch writers (zh_tar_create_batch, zh_zip_write_batch) ----
// Their call-level checks, in this order: the pointers; dsts / dst_lens / statuses cleared; `bad_call` (the code of a
// bad level or format, ZH_OK if none); then the table -- first[] ascending, entries there, every path and contents
// there.  The caller goes on only on ZH_OK with n > 0.
template <class Entry>
static int writer_checks(zh_ctx* ctx, const Entry* entries, const size_t* first, size_t n, int bad_call, void** dsts,
                         size_t* dst_lens, int32_t* statuses) {
  if (!ctx || (n && (!first || !dsts || !dst_lens || !statuses))) return ZH_ERR_ARGUMENT;
  clear_outputs(dsts, dst_lens, statuses, n);
  if (bad_call || !n) return bad_call;
  for (size_t t = 0; t < n; t++)
    if (first[t + 1] < first[t]) return ZH_ERR_ARGUMENT;
  if (first[n] > first[0] && !entries) return ZH_ERR_ARGUMENT;
  for (size_t i = first[0]; i < first[n]; i++)
    if ((!entries[i].path && entries[i].path_len) || (!entries[i].contents && entries[i].len)) return ZH_ERR_ARGUMENT;
  return ZH_OK;
}
// Their results: the device ranges [off[k], + len[k]) of d_img whose st[k] is ZH_OK into fresh buffers, handed out
// with st[k] at batch position pos[k].  Nothing is handed out from a failed call.
static inline int writer_hand_out(zh_ctx* ctx, const uint8_t* d_img, const std::vector<size_t>& pos,
                                  const std::vector<uint64_t>& off, const std::vector<uint64_t>& len,
                                  std::vector<int32_t> st, void** dsts, size_t* dst_lens, int32_t* statuses) {
  const size_t n = pos.size();
  std::vector<void*> odst(n, nullptr);
  std::vector<size_t> olen(n, 0);
  std::vector<char> take(n);
  for (size_t k = 0; k < n; k++) take[k] = st[k] == ZH_OK;
  if (const int e = zhh_download(ctx, d_img, n, off, len, take, odst.data(), olen.data(), st.data())) {
    for (void* p : odst) free(p);
    return e;
  }
  for (size_t k = 0; k < n; k++) {
    dsts[pos[k]] = odst[k];
    dst_lens[pos[k]] = olen[k];
    statuses[pos[k]] = st[k];
  }
  return ZH_OK;
}

// ---- the batch readers (zh_tar_open_batch, zh_tar_read_batch, zh_zip_open_all_batch, zh_zip_read_batch) ----
// Their call-level checks, in this order: the pointers; readers / statuses cleared; every image there.  The caller
// goes on only on ZH_OK with n > 0.
template <class Reader>
static int reader_checks(zh_ctx* ctx, const void* const* images, const size_t* lens, size_t n, Reader** readers,
                         int32_t* statuses) {
  if (!ctx || (n && (!images || !lens || !readers || !statuses))) return ZH_ERR_ARGUMENT;
  for (size_t t = 0; t < n; t++) {
    readers[t] = nullptr;
    statuses[t] = ZH_OK;
  }
  for (size_t t = 0; t < n; t++)
    if (!images[t] && lens[t]) return ZH_ERR_ARGUMENT;
  return ZH_OK;
}

struct HostBufs {  // host buffers of the call that no reader owns yet
  std::vector<void*> p;
  ~HostBufs() {
    for (void* q : p) free(q);
  }
};

struct Events {  // ZH_TRACE: kernels by themselves, between pairs of events that go away with the scope
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  bool ok = false;
  bool create() {
    ok = true;
    for (hipEvent_t& x : e) ok = ok && hipEventCreate(&x) == hipSuccess;
    return ok;
  }
  float ms(int a, int b) const {
    float t = 0;
    return hipEventSynchronize(e[b]) == hipSuccess && hipEventElapsedTime(&t, e[a], e[b]) == hipSuccess ? t : -1.f;
  }
  ~Events() {
    for (hipEvent_t x : e)
      if (x) (void)hipEventDestroy(x);
  }
};

// internal.nim:294-302 verifyPathIsSafeToExtract on the four bytes x of a path that start at position `at` (the
// parse kernels of zh_tar_open_batch.hip and zh_zip_open_batch.hip)
static __device__ __forceinline__ bool unsafe_at(uint32_t x, uint64_t at) {
  if (x == 0x2f2e2e2fu || x == 0x5c2e2e5cu) return true;  // "/../", "\..\"
  if (at != 0) return false;
  return (x & 0xffu) == '/' || (x & 0xffffffu) == 0x2f2e2eu || (x & 0xffffffu) == 0x5c2e2eu;  // "/", "../", "..\"
}
