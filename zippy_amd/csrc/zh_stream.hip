// Streaming compress (zh_compress_stream_batch; the state's layout and the contract -- what the bytes are -- are
// include/zippy_hip.h's): streams compressed piece by piece, every piece a run of whole deflate blocks of its own,
// spliced bit-exactly behind the up to seven bits the call before left over.
// The states, the container's header and trailer and the running checksum are the host's.  Every live piece goes up in
// one upload; the live streams, sorted by (level, block size), run in groups whose slots fit the scratch budget, one
// after the other:
//   (plan)                     ONE raw-deflate compress plan (zh_plan_compress_blocks) over the group's pieces into
//                              scratch slots; CRC-32 by the plan, Adler-32 by the checksum kernels over its pieces
//   zh_stream_consts_kernel    a wave a stream: the first stored block among the plan's block entries (one ballot per
//                              64 of them), hence the two regimes of the splice, the BFINAL bit to clear, the length
//   zh_stream_splice_kernel    a wave a (stream, 4 KiB of output) task: every delivered byte is a function of at most two
//                              slot bytes and the stream's constants -- no atomics, no read-modify-write, no order
//                              between lanes --, whole aligned 16-byte stores from unaligned 16-byte gathers
//                              (zh_gather.h); the task that owns the byte behind the last delivered one writes the
//                              stream's delivered length and its new pending bits
// and one download a group brings lengths, pending bits and data down.  A stream whose piece is empty never reaches the
// device (but to FINISH at HuffmanOnly): its bytes are the header, the marker or the empty final block, the trailer.
#include "zh_gather.h"
#include "zh_host.h"

namespace {

constexpr uint32_t kSpliceTask = 4096;  // output bytes a wave of the splice kernel makes
constexpr uint64_t kNoBit = ~0ull;

struct ZhSpliceStream {  // what the host knows of a live stream
  uint64_t slot;   // its piece's stream in the slots (a multiple of 256)
  uint64_t obase;  // where byte 0 of what it makes lies in the output (behind the room for a header)
  uint64_t cap;    // the slot's size
  uint32_t buf;    // its piece in the group's plan
  uint32_t k;      // pending bits
  uint32_t pend_byte;
  uint32_t flush;
};
struct ZhSpliceConst {  // ... and what zh_stream_consts_kernel finds
  uint64_t end;     // bits of R
  uint64_t lim;     // source bits below this move up by k: p + 3, or `end` without a stored block
  uint64_t seam_d;  // output bytes from here on are whole source bytes (kNoBit: none)
  uint64_t delta;   // ... output byte j = source byte j - delta (0 or 1)
  uint64_t fbit;    // the source bit to clear (kNoBit: none)
  uint64_t dend;    // the output bit behind R's last
  uint64_t total;   // bytes delivered
  uint32_t pend;    // bits left over
  uint32_t ok;
};

// One byte of the output of a stream: `S` its slot, x / c its constants
struct SpliceGen {
  const uint8_t* __restrict__ S;
  ZhSpliceStream x;
  ZhSpliceConst c;
  // source byte i with everything at or above bit `limit` zero and the BFINAL bit cleared; byte -1: the pending bits,
  // at its top
  __device__ __forceinline__ uint32_t sbyte(uint64_t i, uint64_t limit) const {
    if (i == kNoBit) return (x.pend_byte << (8u - x.k)) & 0xffu;
    if (i * 8 >= limit) return 0u;
    uint32_t v = S[i];
    if (limit - i * 8 < 8) v &= (1u << (uint32_t)(limit - i * 8)) - 1u;
    if (c.fbit != kNoBit && (c.fbit >> 3) == i) v &= ~(1u << (uint32_t)(c.fbit & 7u));
    return v;
  }
  __device__ __forceinline__ uint32_t byte(uint64_t j) const {
    if (x.flush == ZH_FLUSH_SYNC) {  // 00 00 FF FF behind three zero bits and the padding
      const uint64_t m = (c.dend + 3 + 7) >> 3;
      if (j >= m + 2) return j < m + 4 ? 0xffu : 0u;
    }
    if (j >= c.seam_d) return sbyte(j - c.delta, c.end);
    const uint32_t v16 = sbyte(j - 1, c.lim) | (sbyte(j, c.lim) << 8);  // (j - 1 of byte 0 is kNoBit)
    return (v16 >> (8u - x.k)) & 0xffu;
  }
};

}  // namespace

// One wave per live stream of the group.  blocks / b_mode / b_start / bufs / status: the plan's.
__global__ __launch_bounds__(64) void zh_stream_consts_kernel(const ZhSpliceStream* __restrict__ streams, uint32_t n,
                                                              const ZhBufDesc* __restrict__ bufs,
                                                              const ZhBlockDesc* __restrict__ blocks,
                                                              const uint32_t* __restrict__ b_mode,
                                                              const uint64_t* __restrict__ b_start, uint32_t nblocks_all,
                                                              const int32_t* __restrict__ status,
                                                              ZhSpliceConst* __restrict__ consts) {
  const uint32_t t = blockIdx.x, lane = zh_lane();
  if (t >= n) return;
  const ZhSpliceStream x = streams[t];
  const ZhBufDesc bd = bufs[x.buf];
  ZhSpliceConst c{};
  c.ok = status[x.buf] == ZH_OK ? 1u : 0u;
  uint64_t end = b_start[nblocks_all + x.buf];
  if (end > x.cap * 8) c.ok = 0u;  // (cannot be: the layout refuses a stream that outgrows its slot)
  if (!c.ok) {
    if (lane == 0) consts[t] = c;  // nothing is delivered
    return;
  }
  // the first stored block: one ballot over 64 of the stream's block entries
  uint32_t first = 0xffffffffu;
  for (uint32_t k0 = 0; k0 < bd.nblocks && first == 0xffffffffu; k0 += 64) {
    const uint32_t k = k0 + lane;
    const bool stored = k < bd.nblocks && b_mode[bd.first_block + k] == ZH_MODE_STORED;
    const uint64_t m = __ballot(stored);
    if (m) first = k0 + (uint32_t)__builtin_ctzll(m);
  }
  c.end = end;
  c.lim = end;
  c.seam_d = kNoBit;
  c.dend = end + x.k;
  if (first != 0xffffffffu) {
    const uint64_t p = b_start[bd.first_block + first];
    const uint64_t seam_s = (p + 3 + 7) >> 3;
    c.lim = p + 3;
    c.seam_d = (p + x.k + 3 + 7) >> 3;
    c.delta = c.seam_d - seam_s;
    c.dend = end + c.delta * 8;
  }
  c.fbit = kNoBit;
  if (x.flush != ZH_FLUSH_FINISH && bd.nblocks) {  // BFINAL of the last block; of a stored one: of its last chunk
    const uint32_t last = bd.first_block + bd.nblocks - 1;
    const uint64_t s0 = b_start[last];
    c.fbit = s0;
    if (b_mode[last] == ZH_MODE_STORED) {
      const uint64_t chunks = (blocks[last].len + ZH_STORED_MAX - 1) / ZH_STORED_MAX;
      if (chunks > 1) c.fbit = (((s0 + 3 + 7) >> 3) + (chunks - 1) * (ZH_STORED_MAX + 5ull) - 1) * 8;
    }
  }
  if (x.flush == ZH_FLUSH_SYNC) {
    c.total = ((c.dend + 3 + 7) >> 3) + 4;
  } else if (x.flush == ZH_FLUSH_FINISH) {
    c.total = (c.dend + 7) >> 3;
  } else {
    c.total = c.dend >> 3;
    c.pend = (uint32_t)(c.dend & 7u);
  }
  if (lane == 0) consts[t] = c;
}

struct ZhSpliceTask {
  uint32_t stream, pad;
  uint64_t lo;  // output bytes [lo, lo + kSpliceTask) of the stream
};

// One wave per task (four a workgroup).  out_len[t] / out_pend[t] (bits | byte << 8): written by the task that owns
// byte `total` of stream t -- the byte the pending bits lie in.
__global__ __launch_bounds__(256) void zh_stream_splice_kernel(const uint8_t* __restrict__ slots,
                                                               uint8_t* __restrict__ d_out,
                                                               const ZhSpliceStream* __restrict__ streams,
                                                               const ZhSpliceConst* __restrict__ consts,
                                                               const ZhSpliceTask* __restrict__ tasks, uint32_t n_tasks,
                                                               uint64_t* __restrict__ out_len,
                                                               uint32_t* __restrict__ out_pend) {
  const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = zh_lane();
  if (w >= n_tasks) return;
  const ZhSpliceTask t = tasks[w];
  const SpliceGen g{slots + streams[t.stream].slot, streams[t.stream], consts[t.stream]};
  const ZhSpliceConst& c = g.c;
  const uint32_t k = g.x.k;
  if (lane == 0 && c.total >= t.lo && c.total < t.lo + kSpliceTask) {
    out_len[t.stream] = c.total;
    out_pend[t.stream] = c.pend | ((c.pend ? g.byte(c.total) & ((1u << c.pend) - 1u) : 0u) << 8);
  }
  if (t.lo >= c.total) return;
  // the task's bytes as addresses of d_out: [a, b); q = obase + j
  const uint64_t ob = g.x.obase, a = ob + t.lo, b = ob + (c.total < t.lo + kSpliceTask ? c.total : t.lo + kSpliceTask);
  const uint64_t A = (a + 15) & ~(uint64_t)15, B = b & ~(uint64_t)15;
  if (A >= B) {  // no whole chunk inside: at most 30 bytes
    if (a + lane < b) d_out[a + lane] = (uint8_t)g.byte(a + lane - ob);
    return;
  }
  if (a + lane < A) d_out[a + lane] = (uint8_t)g.byte(a + lane - ob);
  if (B + lane < b) d_out[B + lane] = (uint8_t)g.byte(B + lane - ob);
  const uint32_t lo_mask = 0x01010101u * ((1u << k) - 1u);  // per byte: the k bits that come from the byte before
  const uint64_t fbyte = c.fbit == kNoBit ? kNoBit : c.fbit >> 3;
  for (uint64_t q = A + 16ull * lane; q < B; q += 1024) {
    const uint64_t j = q - ob;  // the chunk is output bytes [j, j + 16)
    Chunk16 v;
    if (j >= c.seam_d) {
      // whole source bytes [s, s + 16): plain where they all lie below `end` and none holds the bit to clear
      const uint64_t s = j - c.delta;
      if ((s + 16) * 8 <= c.end && !(fbyte != kNoBit && fbyte >= s && fbyte < s + 16))
        v = gather16(g.S, s);
      else
        v = bytes16(g, j);
    } else if (j >= 1 && (c.seam_d == kNoBit || j + 16 <= c.seam_d) && (j + 16) * 8 <= c.lim &&
               !(fbyte != kNoBit && fbyte + 1 >= j && fbyte < j + 16)) {
      // source bytes [j - 1, j + 16), all below `lim`, moved up by k bits
      v = gather16(g.S, j);
      if (k) {
        const Chunk16 u = gather16(g.S, j - 1);
#pragma unroll
        for (int i = 0; i < 4; i++) v.w[i] = ((u.w[i] >> (8u - k)) & lo_mask) | ((v.w[i] << k) & ~lo_mask);
      }
    } else {
      v = bytes16(g, j);
    }
    *reinterpret_cast<Chunk16*>(d_out + q) = v;
  }
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
namespace {

inline uint64_t pad256(uint64_t v) { return (v + 255) & ~(uint64_t)255; }

// ---- the running checksum: crc(A || B) and adler(A || B) from those of A and B and B's length ----
// A copy, word for word, of zh_resume.hip's three functions (file-local there): a change to either is a change to both,
// until they move to a header of their own.
constexpr uint32_t kCrcPoly = 0xedb88320u;
uint32_t crc_mul(uint32_t a, uint32_t b) {  // a(x) * b(x) mod P, reflected (x^0: bit 31)
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    if (a & 0x80000000u) p ^= b;
    a <<= 1;
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}
uint32_t crc32_join(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
  uint32_t x = 0x80000000u, sq = 0x00800000u;  // x^0, x^8: x = x^(8 len_b)
  for (uint64_t n = len_b; n; n >>= 1) {
    if (n & 1) x = crc_mul(sq, x);
    sq = crc_mul(sq, sq);
  }
  return crc_mul(x, crc_a) ^ crc_b;
}
uint32_t adler32_join(uint32_t ad_a, uint32_t ad_b, uint64_t len_b) {
  const uint64_t m = 65521u, s1a = ad_a & 0xffffu, s2a = ad_a >> 16, s1b = ad_b & 0xffffu, s2b = ad_b >> 16;
  const uint64_t s2 = (s2a + s2b + (len_b % m) * ((s1a + m - 1) % m)) % m;
  const uint64_t s1 = (s1a + s1b + m - 1) % m;
  return (uint32_t)((s2 << 16) | s1);
}

// what can be said of a state without compressing (include/zippy_hip.h)
bool state_sound(const void* state, size_t len, zh_stream_state& h) {
  if (len != sizeof(h)) return false;
  memcpy(&h, state, sizeof(h));
  return memcmp(h.magic, ZH_STREAM_MAGIC, 8) == 0 && h.version == ZH_STREAM_VERSION && h.data_format >= ZH_DF_ZLIB &&
         h.data_format <= ZH_DF_DEFLATE && h.level >= -2 && h.level <= 9 && valid_block_bytes(h.block_bytes) &&
         h.phase == 1 && h.pend_bits <= 7 && (h.pend_byte >> h.pend_bits) == 0 && h.reserved == 0;
}

// the container's header as zh_layout_kernel writes it (zippy.nim:22-42, 61-69) -> its length
uint32_t write_head(uint8_t* out, uint32_t fmt, uint32_t fname_len) {
  if (fmt == ZH_DF_GZIP) {
    const uint8_t fixed[10] = {31, 139, 8, 1u << 3, 0, 0, 0, 0, 0, 0};
    memcpy(out, fixed, 10);
    for (uint32_t j = 0; j < fname_len; j++) out[10 + j] = (uint8_t)(97 + j);
    out[10 + fname_len] = 0;
    return 11 + fname_len;
  }
  if (fmt == ZH_DF_ZLIB) {
    const uint32_t cmf = (7u << 4) | 8u;
    out[0] = (uint8_t)cmf;
    out[1] = (uint8_t)(31u - (cmf * 256u) % 31u);
    return 2;
  }
  return 0;
}
// ... and the trailer (zippy.nim:47-58, 71-78) -> its length
uint32_t write_tail(uint8_t* out, uint32_t fmt, uint32_t check, uint64_t total_in) {
  if (fmt == ZH_DF_GZIP) {
    const uint32_t isize = (uint32_t)(total_in & 0xffffffffu);
    for (int j = 0; j < 4; j++) {
      out[j] = (uint8_t)(check >> (8 * j));
      out[4 + j] = (uint8_t)(isize >> (8 * j));
    }
    return 8;
  }
  if (fmt == ZH_DF_ZLIB) {
    for (int j = 0; j < 4; j++) out[j] = (uint8_t)(check >> (8 * (3 - j)));
    return 4;
  }
  return 0;
}
constexpr uint32_t kHeadMax = 36, kTailMax = 8;

struct Live {  // a stream of the call: where it stands before it
  size_t i;
  zh_stream_state h;
  uint8_t head[kHeadMax];
  uint32_t head_len;  // a new stream's header (0: resumed, or raw deflate)
  uint32_t flush;
  uint64_t cap, slot, obase, src_at;
};

void* make_state(const zh_stream_state& h) {
  void* blob = malloc(sizeof(h));
  if (blob) memcpy(blob, &h, sizeof(h));
  return blob;
}

}  // namespace

static_assert(sizeof(zh_stream_state) == 64, "the state's layout is the header's");

// The call; `cleared`: the output arrays have been set (what they hold from then on is the library's to free)
static int stream_run(zh_ctx* ctx, const void* const* srcs, const size_t* lens, size_t n, int level, int data_format,
                      size_t block_bytes, const void* const* states, const size_t* state_lens, const uint8_t* flush,
                      void** dsts, size_t* dst_lens, void** new_states, size_t* new_state_lens, int32_t* statuses,
                      bool& cleared) {
  if (!ctx || (n && (!srcs || !lens || !dsts || !dst_lens || !new_states || !new_state_lens || !statuses)) ||
      (state_lens && !states) || (states && !state_lens))
    return ZH_ERR_ARGUMENT;
  clear_outputs(dsts, dst_lens, statuses, n);
  for (size_t i = 0; i < n; i++) {
    new_states[i] = nullptr;
    new_state_lens[i] = 0;
  }
  cleared = true;
  bool any_new = false;
  for (size_t i = 0; i < n; i++) {
    if ((!srcs[i] && lens[i]) || (flush && flush[i] > ZH_FLUSH_FINISH) || (states && !states[i] && state_lens[i]))
      return ZH_ERR_ARGUMENT;
    if (!states || !states[i]) any_new = true;
  }
  const size_t bb_new = block_bytes ? block_bytes : ZH_BLOCK_SIZE;
  if (any_new) {
    if (level < -2 || level > 9) return ZH_ERR_ARGUMENT;
    if (data_format != ZH_DF_GZIP && data_format != ZH_DF_ZLIB && data_format != ZH_DF_DEFLATE) return ZH_ERR_ARGUMENT;
    if (!valid_block_bytes(bb_new)) return ZH_ERR_ARGUMENT;
  }
  if (!n) return ZH_OK;
  if (n > 0x7fffffffull) return ZH_ERR_ARGUMENT;

  // ---- what the host settles: states, headers, the streams that make no block in this call ----
  std::vector<Live> live;
  for (size_t i = 0; i < n; i++) {
    Live v{};
    v.i = i;
    v.flush = flush ? flush[i] : (uint32_t)ZH_FLUSH_SYNC;
    if (states && states[i]) {
      if (!state_sound(states[i], state_lens[i], v.h)) {
        statuses[i] = ZH_ERR_INVALID_BUFFER;
        continue;
      }
    } else {
      memcpy(v.h.magic, ZH_STREAM_MAGIC, 8);
      v.h.version = ZH_STREAM_VERSION;
      v.h.data_format = (uint32_t)data_format;
      v.h.level = level;
      v.h.block_bytes = (uint32_t)bb_new;
      v.h.phase = 1;
      v.h.check = data_format == ZH_DF_ZLIB ? 1u : 0u;
      int k = ctx->fname_len;
      if (k < 0) k = (int)(ctx->rng() % 26);  // zippy.nim:28-38
      v.head_len = write_head(v.head, (uint32_t)data_format, (uint32_t)k);
    }
    // An empty piece makes no block (BLOCK), the marker (SYNC) or, with FINISH, the reference's block for no input: an
    // empty stored one at every level (deflate.nim:214-226, 275-277) but HuffmanOnly, whose coded block of the
    // end-of-block symbol alone comes from the plan like any other piece's.
    // HAZARD: this also keeps empty buffers out of chain-level plans (-1, 2..9).  There an empty buffer's one block has
    // no fragment, and where ZH_SCRATCH_MB is so small that the block becomes a range of its own
    // (zh_plan_compress_blocks, chain_ranges) the chain kernels are launched over zero fragments: hipGetLastError says
    // "invalid configuration argument" and the whole call fails with ZH_ERR_DEVICE (met on the MI355X with
    // ZH_SCRATCH_MB=1; the emulator does not mind an empty grid).  Whoever routes empty pieces through the plan mends
    // that first.  HuffmanOnly is no chain level, so its empty FINISH is safe.
    if (lens[i] || (v.flush == ZH_FLUSH_FINISH && v.h.level == -2)) {
      live.push_back(v);
      continue;
    }
    uint8_t bytes[kHeadMax + 6 + kTailMax];
    size_t nb = v.head_len;
    if (nb) memcpy(bytes, v.head, nb);
    const bool fin = v.flush == ZH_FLUSH_FINISH;
    if (v.flush != ZH_FLUSH_BLOCK) {
      // BFINAL, BTYPE 00 and the padding behind the pending bits: the rest of their byte, or one more; LEN, NLEN
      bytes[nb++] = (uint8_t)(v.h.pend_byte | (fin ? 1u << v.h.pend_bits : 0u));
      if (v.h.pend_bits + 3 > 8) bytes[nb++] = 0;
      bytes[nb++] = 0;
      bytes[nb++] = 0;
      bytes[nb++] = 0xff;
      bytes[nb++] = 0xff;
      v.h.pend_bits = v.h.pend_byte = 0;
    }
    if (fin) nb += write_tail(bytes + nb, v.h.data_format, v.h.check, v.h.total_in);
    v.h.total_out += nb;
    void* out = nb ? malloc(nb) : nullptr;
    void* blob = fin ? nullptr : make_state(v.h);
    if ((nb && !out) || (!fin && !blob)) {
      free(out);
      free(blob);
      statuses[i] = ZH_ERR_NOMEM;
      continue;
    }
    if (nb) memcpy(out, bytes, nb);
    dsts[i] = out;
    dst_lens[i] = nb;
    new_states[i] = blob;
    new_state_lens[i] = fin ? 0 : sizeof(v.h);
  }
  const size_t nl = live.size();
  if (!nl) return ZH_OK;
  // streams of one level and block size stand together: a plan has one of each
  std::stable_sort(live.begin(), live.end(), [](const Live& a, const Live& b) {
    return a.h.level != b.h.level ? a.h.level < b.h.level : a.h.block_bytes < b.h.block_bytes;
  });

  // ---- the upload: every live piece, each at a multiple of 16 ----
  ZH_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  Trace tr;
  std::vector<const void*> up_src(nl);
  std::vector<uint64_t> up_off(nl), up_len(nl);
  uint64_t up_total = 0;
  for (size_t k = 0; k < nl; k++) {
    Live& v = live[k];
    v.src_at = up_total;
    up_src[k] = srcs[v.i];
    up_off[k] = up_total;
    up_len[k] = lens[v.i];
    up_total = (up_total + lens[v.i] + 15) & ~(uint64_t)15;
  }
  DevBuf d_src;
  if (dev_alloc(ctx, d_src, up_total + 256) != hipSuccess) return ZH_ERR_NOMEM;
  if (up_total)
    if (const int st = zhh_upload_slices(ctx, up_src.data(), up_off, up_len, up_total, d_src.p)) return st;
  tr.mark(ctx, "stream: upload");

  // ---- the groups: streams of one (level, block size) whose slots and output fit the scratch budget ----
  struct Group {
    size_t k0, nk;
    uint64_t slots, outs;
  };
  const uint64_t budget = scratch_budget();
  std::vector<Group> groups;
  {
    Group g{0, 0, 0, 0};
    for (size_t k = 0; k < nl; k++) {
      Live& v = live[k];
      const uint64_t len = lens[v.i], bb = v.h.block_bytes;
      v.cap = zh_compress_bound(len, ZH_DF_DEFLATE) + 1024 * ((len + bb - 1) / bb + 1);
      const uint64_t slot_bytes = pad256(v.cap + kGatherSlack), out_bytes = pad256(kHeadMax + v.cap + 16 + kTailMax);
      const bool same = g.nk && live[g.k0].h.level == v.h.level && live[g.k0].h.block_bytes == v.h.block_bytes;
      if (g.nk && (!same || g.slots + g.outs + slot_bytes + out_bytes > budget)) {
        groups.push_back(g);
        g = Group{k, 0, 0, 0};
      }
      v.slot = g.slots;
      // (what the kernel makes starts behind the header; the host writes header and trailer into the download)
      v.obase = g.outs + v.head_len;
      g.slots += slot_bytes;
      g.outs += out_bytes;
      g.nk++;
    }
    groups.push_back(g);
  }
  if (groups.size() > 1 && getenv("ZH_TRACE"))
    fprintf(stderr, "zippy_hip: stream scratch for %zu groups of streams (%zu streams)\n", groups.size(), nl);

  for (const Group& q : groups) {
    const size_t nk = q.nk;
    const int glevel = live[q.k0].h.level;
    const size_t gbb = live[q.k0].h.block_bytes;
    std::vector<uint64_t> soff(nk), slen(nk), doff(nk), dcap(nk);
    std::vector<ZhSpliceStream> xs(nk);
    std::vector<ZhSpliceTask> tasks;
    bool any_gzip = false, any_zlib = false;
    for (size_t j = 0; j < nk; j++) {
      const Live& v = live[q.k0 + j];
      soff[j] = v.src_at;
      slen[j] = lens[v.i];
      doff[j] = v.slot;
      dcap[j] = v.cap;
      xs[j] = ZhSpliceStream{v.slot, v.obase, v.cap, (uint32_t)j, v.h.pend_bits, v.h.pend_byte, v.flush};
      // (what is delivered is at most the slot's bytes, one for the pending bits' move, five of marker)
      for (uint64_t lo = 0; lo < v.cap + 8; lo += kSpliceTask) tasks.push_back(ZhSpliceTask{(uint32_t)j, 0, lo});
      any_gzip = any_gzip || v.h.data_format == ZH_DF_GZIP;
      any_zlib = any_zlib || v.h.data_format == ZH_DF_ZLIB;
      if (tasks.size() >= 0x7fffffffull) return ZH_ERR_ARGUMENT;
    }
    const size_t n_task = tasks.size();
    DevBuf d_slots, d_out, d_ar;
    PlanGuard pg;
    int st;
    if (dev_alloc(ctx, d_slots, q.slots + 256) != hipSuccess || dev_alloc(ctx, d_out, q.outs + 256) != hipSuccess) {
      (void)hipGetLastError();
      ctx->last_error = "hipMalloc(stream)";
      return ZH_ERR_NOMEM;
    }
    if ((st = zh_plan_compress_blocks(ctx, nk, soff.data(), slen.data(), doff.data(), dcap.data(), glevel, ZH_DF_DEFLATE,
                                      gbb, &pg.p)) ||
        (any_gzip && (st = zh_plan_request_crc32(pg.p, 1))))
      return st;
    zh_plan* p = pg.p;
    const ZhSpliceStream* d_xs;
    const ZhSpliceTask* d_tasks;
    ZhSpliceConst* d_consts;
    uint64_t* d_olen;
    uint32_t* d_pend;
    Arena ar;
    ar.add(d_xs, nk, xs.data());
    ar.add(d_tasks, n_task, tasks.data());
    ar.add(d_consts, nk);
    ar.add(d_olen, nk);
    ar.add(d_pend, nk);
    ar.pad(256);
    if (ar.alloc(ctx, d_ar) != hipSuccess) return ZH_ERR_NOMEM;
    ar.bind();
    ZH_HIP(ctx, ar.upload(s));
    ZH_HIP(ctx, ar.clear(d_olen, s));
    ZH_HIP(ctx, ar.clear(d_pend, s));
    Events ev;
    const bool timed = tr.on && ev.create();
    if (timed) (void)hipEventRecord(ev.e[0], s);
    if ((st = zh_plan_run(p, d_src.p, d_slots.p))) return st;
    if (any_zlib) {  // (the plan of a raw stream makes no Adler-32: its pieces through the same kernels)
      zh_launch_checksum_pieces(s, ctx->cktabs, d_src.p, p->d_pieces, p->npieces, nullptr, 0, 1, p->piece_crc,
                                p->piece_adler, p->piece_len);
      zh_launch_checksum_combine(s, ctx->cktabs, p->d_bufs, (uint32_t)nk, p->piece_crc, p->piece_adler, p->piece_len, 0, 1,
                                 p->buf_crc, p->buf_adler);
    }
    if (timed) (void)hipEventRecord(ev.e[1], s);
    {
      const ZhBufDesc* const pbufs = p->d_bufs;
      const ZhBlockDesc* const pblocks = p->ca.blocks;
      const uint32_t* const pmode = p->ca.b_mode;
      const uint64_t* const pstart = p->ca.b_start;
      const int32_t* const pstatus = p->status;
      const uint32_t nb_all = p->ca.nblocks;
      const uint8_t* const slots = d_slots.p;
      uint8_t* const outp = d_out.p;
      const ZhSpliceConst* const consts = d_consts;
      hipLaunchKernelGGL(zh_stream_consts_kernel, dim3((uint32_t)nk), dim3(64), 0, s, d_xs, (uint32_t)nk, pbufs, pblocks,
                         pmode, pstart, nb_all, pstatus, d_consts);
      hipLaunchKernelGGL(zh_stream_splice_kernel, dim3(((uint32_t)n_task + 3) / 4), dim3(256), 0, s, slots, outp, d_xs,
                         consts, d_tasks, (uint32_t)n_task, d_olen, d_pend);
    }
    if (timed) (void)hipEventRecord(ev.e[2], s);
    ZH_HIP(ctx, hipGetLastError());
    std::vector<uint64_t> olen(nk);
    std::vector<uint32_t> pend(nk), crc(nk, 0), adler(nk, 1);
    std::vector<int32_t> pst(nk);
    ZH_HIP(ctx, hipMemcpyAsync(olen.data(), d_olen, nk * 8, hipMemcpyDeviceToHost, s));
    ZH_HIP(ctx, hipMemcpyAsync(pend.data(), d_pend, nk * 4, hipMemcpyDeviceToHost, s));
    ZH_HIP(ctx, hipMemcpyAsync(pst.data(), p->status, nk * 4, hipMemcpyDeviceToHost, s));
    if (any_gzip) ZH_HIP(ctx, hipMemcpyAsync(crc.data(), p->buf_crc, nk * 4, hipMemcpyDeviceToHost, s));
    if (any_zlib) ZH_HIP(ctx, hipMemcpyAsync(adler.data(), p->buf_adler, nk * 4, hipMemcpyDeviceToHost, s));
    ZH_HIP(ctx, hipStreamSynchronize(s));
    if (timed)
      fprintf(stderr, "[zh] stream: plan %.3f ms, splice %.3f ms (%zu streams, %zu tasks)\n", ev.ms(0, 1), ev.ms(1, 2), nk,
              n_task);
    tr.mark(ctx, "stream: compress + splice");

    // ---- the group's data, with room for header and trailer around what the kernel made ----
    std::vector<uint64_t> g_off(nk), g_len(nk);
    std::vector<char> take(nk);
    std::vector<void*> gd(nk, nullptr);
    std::vector<size_t> gl(nk, 0);
    std::vector<int32_t> gs(nk, ZH_OK);
    for (size_t j = 0; j < nk; j++) {
      const Live& v = live[q.k0 + j];
      const uint64_t made = std::min<uint64_t>(olen[j], v.cap + 8);
      const uint64_t tail = v.flush == ZH_FLUSH_FINISH ? (v.h.data_format == ZH_DF_GZIP ? 8u : v.h.data_format == ZH_DF_ZLIB ? 4u : 0u) : 0u;
      g_off[j] = v.obase - v.head_len;
      g_len[j] = v.head_len + made + tail;
      take[j] = pst[j] == ZH_OK && g_len[j] != 0;
    }
    if (const int e = zhh_download(ctx, d_out.p, nk, g_off, g_len, take, gd.data(), gl.data(), gs.data())) {
      for (void* b : gd) free(b);
      return e;
    }
    tr.mark(ctx, "stream: download");

    // ---- the group's streams settled: header, running checksum, trailer, the state to come back with ----
    for (size_t j = 0; j < nk; j++) {
      const Live& v = live[q.k0 + j];
      const size_t i = v.i;
      uint8_t* data = (uint8_t*)gd[j];
      if (pst[j] != ZH_OK || gs[j] != ZH_OK) {
        free(data);
        statuses[i] = pst[j] != ZH_OK ? pst[j] : gs[j];
        continue;
      }
      zh_stream_state h = v.h;
      if (lens[i]) {
        if (h.data_format == ZH_DF_GZIP) h.check = crc32_join(h.check, crc[j], lens[i]);
        else if (h.data_format == ZH_DF_ZLIB) h.check = adler32_join(h.check, adler[j], lens[i]);
      }
      h.total_in += lens[i];
      h.total_out += g_len[j];
      h.pend_bits = pend[j] & 0xffu;
      h.pend_byte = pend[j] >> 8;
      if (data && v.head_len) memcpy(data, v.head, v.head_len);
      if (v.flush == ZH_FLUSH_FINISH) {
        if (data) write_tail(data + (g_len[j] - (h.data_format == ZH_DF_GZIP ? 8u : h.data_format == ZH_DF_ZLIB ? 4u : 0u)),
                             h.data_format, h.check, h.total_in);
      } else {
        void* blob = make_state(h);
        if (!blob) {
          free(data);
          statuses[i] = ZH_ERR_NOMEM;
          continue;
        }
        new_states[i] = blob;
        new_state_lens[i] = sizeof(h);
      }
      dsts[i] = data;
      dst_lens[i] = take[j] ? g_len[j] : 0;
    }
  }
  return ZH_OK;
}

// A call that fails as a whole hands nothing out: whatever the groups before the failure had settled is freed.
extern "C" int zh_compress_stream_batch(zh_ctx* ctx, const void* const* srcs, const size_t* lens, size_t n, int level,
                                        int data_format, size_t block_bytes, const void* const* states,
                                        const size_t* state_lens, const uint8_t* flush, void** dsts, size_t* dst_lens,
                                        void** new_states, size_t* new_state_lens, int32_t* statuses) {
  bool cleared = false;
  const int rc = stream_run(ctx, srcs, lens, n, level, data_format, block_bytes, states, state_lens, flush, dsts, dst_lens,
                            new_states, new_state_lens, statuses, cleared);
  if (rc != ZH_OK && cleared)
    for (size_t i = 0; i < n; i++) {
      free(dsts[i]);
      free(new_states[i]);
      dsts[i] = new_states[i] = nullptr;
      dst_lens[i] = new_state_lens[i] = 0;
    }
  return rc;
}
