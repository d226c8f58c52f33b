// The wave-pair inflate: the body of zh_inflate_kernel (zh_inflate.hip: batches, the blocks of block-indexed streams)
// and of zh_seek_inflate_kernel (zh_seek.hip: the intervals of a seek index).  Each kernel is alone in its file: with
// both in one, the table builder and the slow symbol path had two callers, were no longer inlined, and the existing
// kernel took 176 bytes of scratch a lane instead of 72.  A third form, zh_resume_inflate_kernel (zh_resume.hip), does
// not know where it will stop: it decodes whole blocks until the input or the output budget gives out.
#pragma once
#include "zh_common.h"
#include "zh_kprof.h"
#include "zh_tables.h"
#include "zh_inflate_header.h"

// Two waves per stream, one producer and one consumer, a barrier per round:
//
// DECODE wave: owns the bit stream.  A round covers up to 128 bit positions: lane l decodes
//   the whole tokens -- literal, or length + extra + distance + extra -- that WOULD start l
//   and 64 + l bits behind the current position, each from its own 64-bit view of the stream
//   (two LDS lookups, inflate.nim:93-100 / 199-222 for all offsets at once).  A wave-uniform
//   walk then follows the real chain of token starts through those lanes (seven instructions
//   per symbol), DPP prefix sums of the chain's output lengths place every token, and the
//   round goes into one of two descriptor buffers in LDS.  Anything the LUTs cannot finish in
//   the lane (codes past the tables' reach, end of block, invalid symbols) stops the chain and is decoded alone
//   with the canonical slow path (inflate.nim:67-91) as the round's "tail".  Block headers,
//   table construction and stored blocks happen here too.
// OUTPUT wave: owns the output.  Rounds of <= 64 bytes (the usual case) get one lane per
//   OUTPUT byte: token starts are scattered by output offset and a running maximum tells
//   every byte its token; literals carry their value, match bytes read earlier output back
//   through L2 (the LZ window is the output itself), bytes copied from the round's own output
//   chase their source down by pointer doubling -- inflate.nim:227-250's byte-sequential copy
//   semantics without a loop over the tokens.  Longer rounds run their copies in order.
// While the output wave works on round k the decode wave is already on round k + 1.
namespace {

constexpr uint32_t kTailNone = 0, kTailLiteral = 1, kTailMatch = 2, kTailStored = 3, kTailEnd = 4;
// the resuming form: the decode wave stands at a block boundary, tail_off: its bit position, tail_a: the block before
// it was the final one
constexpr uint32_t kTailMark = 5;
// the forms of the body, and the status with which the resuming form's decode wave says "the input ends here"
constexpr int kFormBatch = 0, kFormSeek = 1, kFormResume = 2;
constexpr int kStNeedInput = 1000;

struct RoundDesc {
  // per lane and window: output length (9) | literal << 9 | in chain << 10 | value << 16
  // (value: the literal byte, or the match distance)
  uint32_t rec[2][64];
  uint32_t use_b;    // window B holds tokens too
  uint32_t tail;     // what follows the chain (kTail*)
  uint32_t tail_a;   // literal byte | match length | stored length | final status
  uint32_t tail_b;   // match distance
  uint64_t tail_off; // stored run: offset of its first byte in the compressed stream
};

}  // namespace

// kSeek: an interval of a seek index (zh_seek.hip, ZhSeekStop x): the slot already holds
// hist_len bytes of history, so the output wave starts with op = hist_len and inflate.nim:224-225's `distance > op`
// keeps its meaning -- the LZ window remains the output itself --; the decode wave ends at the top of the block loop
// where its position is stop_bit, and a position beyond it, or a final block that ends elsewhere, is
// ZH_ERR_INVALID_BUFFER.  out_len counts the history.  A kernel of its own, zh_seek_inflate_kernel (zh_seek.hip): the
// kernel of the batches and of the block-indexed forms, zh_inflate_kernel, keeps its name and its arguments.
//
// kFormResume (zh_resume.hip, ZhResume r): history in front of the slot as above, no stop bit.  At the top of the block
// loop, and behind the final block, the decode wave hands the output wave a boundary mark (kTailMark); the output wave
// records (bit, bytes made) when it comes by the mark in round order, so the last record is the last block that was
// decoded AND written whole.  The end of the input and a full slot are no failures here: they end the stream with that
// last boundary and the reason (ZH_RESUME_*), the earlier event in stream order deciding -- the output wave's status
// is raised in round order and outranks the status the decode wave sends with kTailEnd.  Unless r.last[sid] is set,
// no check is decided by a bit at or beyond the end of the input: a field, a code or a token that the end cuts (a
// pattern without a code counts as 7 bits in the code-length code, 15 in the others) answers kStNeedInput, and the
// tokens of a round that the end cuts never reach the output wave.  With r.last[sid] the checks read zeros behind the
// end and give the statuses of the other forms; a token that the end cuts is kept from the output wave all the same.
template <int kForm>
__device__ __forceinline__ void zh_inflate_body(const uint8_t* __restrict__ d_src, uint8_t* __restrict__ d_dst,
                                                const ZhInflateArgs& a, const ZhSeekStop& x, const ZhResume& r) {
  constexpr bool kSeek = kForm == kFormSeek;
  constexpr bool kResume = kForm == kFormResume;
  __shared__ uint32_t s_lit[(1u << kLitBits) + kLitSub];
  __shared__ uint32_t s_dst[1u << kDistBits];  // also hosts the 7-bit code-length table
  __shared__ uint32_t s_in[kInWords];          // staging ring of the compressed stream
  __shared__ uint8_t s_map[64];                // output byte -> token lane of the current round
  __shared__ HuffTab s_tab_lit, s_tab_dist, s_tab_cl;
  __shared__ uint16_t s_val_lit[288], s_val_dist[32], s_val_cl[20];
  __shared__ uint8_t s_lens[320 + 16];
  __shared__ uint32_t s_cnt[16];
  __shared__ RoundDesc s_desc[2];
  __shared__ int32_t s_ostatus;  // raised by the output wave, polled by the decode wave

  const unsigned lane = zh_lane();
  const bool decoder = threadIdx.x < 64;
  const uint32_t sid = blockIdx.x;
  if (a.status[sid] != ZH_OK) return;  // unwrap already failed this stream (both waves leave)
  if (a.skip && a.skip[sid]) return;  // decoded (or sized) segment-wise, zh_inflate_seg.hip

  const ZhBufDesc bd = a.bufs[sid];
  const uint8_t* src = d_src + bd.src_off;
  const uint64_t src_len = a.src_len_dev ? a.src_len_dev[sid] : bd.src_len;
  uint8_t* dst = d_dst + bd.dst_off;
  const uint64_t cap = bd.dst_cap;
  const int count_only = a.count_only;
  const uint32_t mis = (uint32_t)((uintptr_t)src & 3u);
  const uint32_t* asrc = reinterpret_cast<const uint32_t*>(src - mis);
  if (threadIdx.x == 0) s_ostatus = ZH_OK;
  __syncthreads();

  if (!decoder) {
    // =========================== OUTPUT wave ===========================
    KPROF_DECL(8);  // output wave: 0 waiting for a round, 1 working; 2 rounds; 3 waves; 4 long rounds; 5 far rounds; 6 doubling turns; 7 tail matches
    uint64_t op = kSeek ? x.hist_len[sid] : 0;  // bytes produced (kSeek: behind the history the slot came with)
    if constexpr (kResume) op = r.hist_len[sid];
    uint64_t mark_bit = 0, mark_op = op;  // kResume: the last block boundary the output has reached
    uint32_t mark_final = 0;
    int st = ZH_OK;
    // match sources are read back past this CU's L1 (which may hold a stale copy of a line the
    // wave has since extended), after the wave's earlier stores have completed
    auto own_output_visible = [&]() {
      zh_wave_sync();  // (lanes read what other lanes stored: a rendezvous for the emulator)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    };
    auto ld_out = [&](uint64_t at) -> uint32_t {
      return __hip_atomic_load(dst + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    // inflate.nim:224-250: one LZ copy of `length` bytes from `dist` back, at op (wave-uniform)
    auto lz_copy = [&](uint32_t length, uint32_t dist) {
      if (dist > op) {  // inflate.nim:224-225
        st = ZH_ERR_INVALID_BUFFER;
        return;
      }
      if (!count_only) {
        if (op + length > cap) {
          st = ZH_ERR_DST_TOO_SMALL;
          return;
        }
        // an overlapping copy (dist < length) repeats the dist-byte pattern, so every lane
        // reads its source from the region already written
        own_output_visible();
        const uint64_t sb = op - dist;
        if (dist >= length) {
          for (uint32_t i = lane; i < length; i += 64) dst[op + i] = (uint8_t)ld_out(sb + i);
        } else if (dist == 1) {
          const uint8_t v = (uint8_t)ld_out(sb);
          for (uint32_t i = lane; i < length; i += 64) dst[op + i] = v;
        } else {
          for (uint32_t i = lane; i < length; i += 64) dst[op + i] = (uint8_t)ld_out(sb + i % dist);
        }
      }
      op += length;
    };
    for (uint32_t k = 0;; k++) {
      KPROF_MARK(1);
      __syncthreads();  // round k is in s_desc[k & 1]
      KPROF_MARK(0);
      KPROF_COUNT(2, 1);
      // wave-uniform by construction; saying so keeps them in scalar registers and the control
      // flow below on scalar branches
      op = zh_bcast64(op);
      st = (int)zh_bcast((uint32_t)st);
      const RoundDesc& d = s_desc[k & 1u];
      const uint32_t use_b = d.use_b, tail = d.tail, tail_a = d.tail_a, tail_b = d.tail_b;
      const uint64_t tail_off = d.tail_off;
      const uint32_t recA = d.rec[0][lane];
      const uint32_t recB = use_b ? d.rec[1][lane] : 0u;
      if (tail == kTailEnd) {
        if (st == ZH_OK) st = (int)tail_a;
        break;
      }
      if (st != ZH_OK) continue;  // failed: keep taking rounds until the decode wave stops
      if constexpr (kResume) {
        if (tail == kTailMark) {
          mark_bit = tail_off;
          mark_op = op;
          mark_final = tail_a;
          continue;
        }
      }
      // where every token's output goes: prefix sums of the chain's output lengths
      const bool in_chain = (recA >> 10) & 1u, is_lit = (recA >> 9) & 1u;
      const bool in_chainB = (recB >> 10) & 1u, is_litB = (recB >> 9) & 1u;
      const uint32_t valA = recA >> 16, valB = recB >> 16;
      const uint32_t lenA = in_chain ? recA & 0x1ffu : 0u, lenB = in_chainB ? recB & 0x1ffu : 0u;
      // one scan for both windows: A's lengths in the low half, B's in the high half (a window's
      // sum is at most 64 * 258)
      const uint32_t incl = zh_wave_scan(lenA | (lenB << 16));
      const uint32_t sums = (uint32_t)__builtin_amdgcn_readlane(incl, 63);
      const uint32_t totalA = sums & 0xffffu, totalB = sums >> 16;
      const uint32_t opre = (incl & 0xffffu) - lenA;
      const uint32_t opreB = totalA + (incl >> 16) - lenB;
      const uint32_t total = totalA + totalB;
      if (total - 1u < 64u) {
        const bool is_match = in_chain && !is_lit, is_matchB = in_chainB && !is_litB;
        // inflate.nim:224-225 `distance > op`: a distance is at most 32768 (30 codes), so the lanes
        // only need asking while the stream is that young
        if (op < 32768u && __ballot((is_match && (uint64_t)valA > op + opre) ||
                                    (is_matchB && (uint64_t)valB > op + opreB))) {
          st = ZH_ERR_INVALID_BUFFER;
        } else if (!count_only && op + total > cap) {
          st = ZH_ERR_DST_TOO_SMALL;
        } else if (!count_only) {
          zh_wave_sync();
          s_map[lane] = 0;
          zh_wave_sync();
          if (in_chain) s_map[opre] = (uint8_t)(lane + 1u);
          if (in_chainB) s_map[opreB] = (uint8_t)(lane + 65u);
          zh_wave_sync();
          const uint32_t tk = zh_wave_scan_max(s_map[lane]);  // token (window, lane) + 1 of output byte `lane`
          const uint32_t j = (tk - 1u) & 63u;
          // both windows' tokens of a lane travel in one cross-lane fetch: 16 bits each, a distance
          // (<= 0x8000) as it is, a literal as 0x9000 | byte
          const uint32_t f1 = (is_lit ? 0x9000u | valA : valA) | ((is_litB ? 0x9000u | valB : valB) << 16);
          const uint32_t g2 = (uint32_t)__shfl((int)f1, (int)j, 64);
          const uint32_t gd = tk > 64u ? g2 >> 16 : g2 & 0xffffu;
          const bool live = lane < total;
          uint32_t val = gd & 0xffu;
          uint32_t par = lane;  // source byte inside this round (itself: a root)
          bool far = false;
          uint32_t back = 0;
          if (live && gd < 0x9000u) {
            if (gd <= lane) {
              par = lane - gd;
            } else {
              back = gd - lane;  // bytes before this round's first
              far = true;
            }
          }
          if (__ballot(far)) {
            KPROF_COUNT(5, 1);
            own_output_visible();
            if (far) val = ld_out(op - back);
          }
          if (__ballot(par != lane)) {
            for (;;) {
              KPROF_COUNT(6, 1);
              const uint32_t pp = (uint32_t)__shfl((int)par, (int)par, 64);
              const bool changed = pp != par;
              par = pp;
              if (!__ballot(changed)) break;
            }
            val = (uint32_t)__shfl((int)val, (int)par, 64);
          }
          if (live) dst[op + lane] = (uint8_t)val;
        }
        // a failed stream reports the bytes it really wrote (out_len <= cap): `op` stops at the
        // last round that fitted
        if (st == ZH_OK) op += total;
      } else if (total) {
        // long rounds: per window, literal runs by their lanes and copies in order
        KPROF_COUNT(4, 1);
        const uint64_t op0 = op;
        auto long_window = [&](bool chain_w, bool lit_w, uint32_t rec_w, uint32_t opre_w) {
          const uint64_t litmask = __ballot(chain_w && lit_w);
          uint64_t mm = __ballot(chain_w && !lit_w);
          uint32_t done_lanes = 0;  // chain lanes below this bit offset are finished
          while (mm && st == ZH_OK) {
            const uint32_t g = (uint32_t)__ffsll((long long)mm) - 1u;
            mm &= mm - 1;
            const uint64_t grp = litmask & ((1ull << g) - 1ull) & (~0ull << done_lanes);
            if (grp) {
              const uint32_t nl = (uint32_t)__popcll(grp);
              if (!count_only) {
                if (op + nl > cap) { st = ZH_ERR_DST_TOO_SMALL; break; }
                if ((grp >> lane) & 1ull) dst[op0 + opre_w] = (uint8_t)(rec_w >> 16);
              }
              op += nl;
            }
            const uint32_t r = __builtin_amdgcn_readlane(rec_w, g);
            lz_copy(r & 0x1ffu, r >> 16);
            done_lanes = g + 1u;
          }
          if (st == ZH_OK) {
            const uint64_t grp = done_lanes < 64u ? litmask & (~0ull << done_lanes) : 0ull;
            if (grp) {
              const uint32_t nl = (uint32_t)__popcll(grp);
              if (!count_only) {
                if (op + nl > cap) st = ZH_ERR_DST_TOO_SMALL;
                else if ((grp >> lane) & 1ull) dst[op0 + opre_w] = (uint8_t)(rec_w >> 16);
              }
              if (st == ZH_OK) op += nl;
            }
          }
        };
        long_window(in_chain, is_lit, recA, opre);
        if (use_b && st == ZH_OK) long_window(in_chainB, is_litB, recB, opreB);
      }
      if (st == ZH_OK) {
        if (tail == kTailLiteral) {
          if (!count_only) {
            if (op + 1 > cap) st = ZH_ERR_DST_TOO_SMALL;
            else if (lane == 0) dst[op] = (uint8_t)tail_a;
          }
          if (st == ZH_OK) op += 1;
        } else if (tail == kTailMatch) {
          KPROF_COUNT(7, 1);
          lz_copy(tail_a, tail_b);
        } else if (tail == kTailStored) {  // inflate.nim:252-266: tail_a raw bytes
          if (!count_only) {
            if (op + tail_a > cap) {
              st = ZH_ERR_DST_TOO_SMALL;
            } else {
              const uint8_t* raw = reinterpret_cast<const uint8_t*>(asrc) + tail_off;
              for (uint32_t i = lane; i < tail_a; i += 64) dst[op + i] = raw[i];
            }
          }
          if (st == ZH_OK) op += tail_a;
        }
      }
      if (st != ZH_OK && lane == 0) s_ostatus = st;
    }
    if (st == ZH_OK && op > cap && !count_only) st = ZH_ERR_DST_TOO_SMALL;
    if constexpr (kResume) {
      // what was delivered: the bytes behind the history up to the last boundary; why the stream stopped there
      int why = -1;
      if (st == ZH_OK && mark_final) why = ZH_RESUME_DONE;
      else if (st == kStNeedInput) why = ZH_RESUME_NEED_INPUT;
      else if (st == ZH_ERR_DST_TOO_SMALL) why = ZH_RESUME_NEED_OUTPUT;
      if (lane == 0) {
        a.out_len[sid] = mark_op - r.hist_len[sid];
        a.status[sid] = why >= 0 ? (int)ZH_OK : st == ZH_OK ? (int)ZH_ERR_INVALID_BUFFER : st;
        r.bit[sid] = mark_bit - (uint64_t)mis * 8;
        r.why[sid] = why >= 0 ? why : 0;
      }
    } else if (lane == 0) {
      a.out_len[sid] = op;
      a.status[sid] = st;
    }
    KPROF_COUNT(3, 1);
    KPROF_FLUSH(16, 8);
    return;
  }

  // =========================== DECODE wave ===========================
  // (it is the critical one of the pair at equal priority -- the output wave waits a fifth of
  // the time -- so its decode + chain walk take first pick of the SIMD's issue slots, below)
  // input: the stream is addressed in bits from the 4-byte aligned base below `src`; 64 dwords
  // at a time go through a 512-byte LDS ring (bitstreams.nim:22-49's refill)
  const uint64_t end = mis + src_len;  // first byte offset (from asrc) past the stream
  auto load_dword = [&](uint64_t off) -> uint32_t { return load_dword_end(asrc, off, end); };
  uint64_t bp = 0;      // stream position in bits (from asrc)
  uint64_t in_hi = 0;   // dwords below in_hi are staged (the ring holds the last kInWords of them)
  uint32_t wnxt = 0;    // lane l: dword in_hi + l, loaded ahead of its use
  auto stage = [&]() {
    zh_wave_sync();
    s_in[(uint32_t)(in_hi + lane) & (kInWords - 1u)] = wnxt;
    in_hi += 64;
    wnxt = load_dword((in_hi + lane) * 4);
    zh_wave_sync();
  };
  auto seek = [&](uint64_t bitpos) {  // restart the staging at bitpos
    bp = bitpos;
    in_hi = bitpos >> 5;
    wnxt = load_dword((in_hi + lane) * 4);
    stage();
  };
  auto ensure = [&]() {  // the round below reads up to five dwords from bp >> 5
    if (in_hi < (bp >> 5) + 8u) stage();
  };
  auto fetch = [&]() -> uint64_t {  // the 64 stream bits at bp (wave-uniform)
    ensure();
    const uint32_t wi = (uint32_t)(bp >> 5), sh = (uint32_t)bp & 31u;
    const uint32_t d0 = zh_bcast(s_in[wi & (kInWords - 1u)]), d1 = zh_bcast(s_in[(wi + 1u) & (kInWords - 1u)]),
                   d2 = zh_bcast(s_in[(wi + 2u) & (kInWords - 1u)]);
    return (uint64_t)zh_alignbit(d1, d0, sh) | ((uint64_t)zh_alignbit(d2, d1, sh) << 32);
  };
  // The header bit reader (hb caches the bits at bp) and, in the block loop below, the header itself: a copy of
  // BlockHeaderReader (zh_inflate_header.h: the same checks in the same order; keep the two alike).  With the shared
  // reader this kernel took 3 % longer on the indexed form, where a block's latency is the kernel's time
  // (profiles/inflate_header_ab.json), so it keeps its own.
  uint64_t hb = 0;
  uint32_t hc = 0;
  auto need = [&]() {
    if (hc < 32u) {
      hb = fetch();
      hc = 64;
    }
  };
  auto take = [&](uint32_t nbits) -> uint32_t {  // nbits <= 16, after need()
    const uint32_t v = (uint32_t)hb & ((1u << nbits) - 1u);
    hb >>= nbits;
    hc -= nbits;
    bp += nbits;
    return v;
  };
  auto past_end = [&]() -> bool { return bp > end * 8; };  // the role of `bitsBuffered < 0`
  // kResume: the caller promised no more input / a check that needs the bits below `need_bit` cannot be decided yet
  bool lastf = false;
  if constexpr (kResume) lastf = r.last[sid] != 0;
  auto short_of = [&](uint64_t need_bit) -> bool { return kResume && !lastf && need_bit > end * 8; };
  KPROF_DECL(8);  // decode wave: 0 waiting for the output wave, 1 other work; 2 rounds; 3 waves; 4 vector decode; 5 chain walks; 6 staging
  uint32_t rk = 0;  // rounds handed over so far
  int st = ZH_OK;
  // hand a round without chain tokens to the output wave
  auto send_tail = [&](uint32_t tail, uint32_t ta, uint32_t tb, uint64_t toff) {
    RoundDesc& d = s_desc[rk & 1u];
    d.rec[0][lane] = 0;
    if (lane == 0) {
      d.use_b = 0;
      d.tail = tail;
      d.tail_a = ta;
      d.tail_b = tb;
      d.tail_off = toff;
    }
    KPROF_MARK(1);
    __syncthreads();
    KPROF_MARK(0);
    rk++;
    if (st == ZH_OK && s_ostatus != ZH_OK) st = s_ostatus;
  };

  // a whole stream starts at its deflate body; a block of an indexed stream at its own first bit
  seek(a.start_bit ? (uint64_t)mis * 8 + a.start_bit[sid] : ((uint64_t)mis + a.body_pos[sid]) * 8);
  const bool single_block = a.single_block != 0;
  bool final_block = false;
  const uint64_t stop_at = kSeek ? (uint64_t)mis * 8 + x.stop_bit[sid] : 0;
  while (!final_block && st == ZH_OK) {  // inflate.nim:273-289
    if (kSeek && bp >= stop_at) {
      if (bp > stop_at) st = ZH_ERR_INVALID_BUFFER;
      break;
    }
    if constexpr (kResume) send_tail(kTailMark, 0, 0, bp);
    hc = 0;
    need();
    const uint32_t bfinal = take(1), btype = take(2);
    if (short_of(bp)) { st = kStNeedInput; break; }
    if (bfinal || single_block) final_block = true;

    if (btype == 0) {  // inflate.nim:252-266 inflateNoCompression
      bp = (bp + 7u) & ~(uint64_t)7;
      hc = 0;
      need();
      const uint32_t len = take(16), nlen = take(16);
      if (short_of(bp)) { st = kStNeedInput; break; }
      if (len + nlen != 65535u) { st = ZH_ERR_INVALID_BUFFER; break; }
      const uint64_t byte_pos = bp >> 3;  // from asrc
      if (byte_pos + len > end) { st = kResume && !lastf ? kStNeedInput : (int)ZH_ERR_END_OF_BUFFER; break; }
      send_tail(kTailStored, len, 0, byte_pos);
      seek((byte_pos + len) * 8);
      continue;
    }
    if (btype == 3) { st = ZH_ERR_BLOCK_HEADER; break; }

    uint32_t hlit = 288, hdist = 30;
    if (btype == 1) {  // fixed codes, inflate.nim:111-113 (rebuilt per block like the reference)
      zh_wave_sync();
      for (uint32_t s = lane; s < 288; s += 64) s_lens[s] = (uint8_t)(s <= 143 ? 8 : s <= 255 ? 9 : s <= 279 ? 7 : 8);
      if (lane < 30) s_lens[288 + lane] = 5;
    } else {  // dynamic header, inflate.nim:115-171
      hlit = take(5) + 257;
      hdist = take(5) + 1;
      const uint32_t hclen = take(4) + 4;
      if (short_of(bp)) { st = kStNeedInput; break; }
      if (hlit > 286 || hdist > 30) { st = ZH_ERR_INVALID_BUFFER; break; }
      zh_wave_sync();
      if (lane < 20) s_lens[lane] = 0;
      zh_wave_sync();
      for (uint32_t i = 0; i < hclen; i++) {
        need();
        const uint32_t v = take(3);
        if (lane == 0) s_lens[c_clcl_order[i]] = (uint8_t)v;
      }
      if (short_of(bp)) { st = kStNeedInput; break; }
      st = build_table(s_lens, 19, s_dst, 7, 2, &s_tab_cl, s_val_cl, s_cnt);
      if (st != ZH_OK) break;
      uint32_t i = 0;
      const uint32_t total = hlit + hdist;
      uint32_t prev = 0;
      while (i != total) {
        need();
        uint32_t sym;
        const uint32_t e = zh_bcast(s_dst[(uint32_t)hb & 127u]);
        if (e) {
          take(e & 15u);
          sym = e >> 16;
        } else {
          uint32_t nb;
          sym = decode_symbol_slow<true>((uint32_t)hb, 7, &s_tab_cl, s_val_cl, &nb);
          take(nb);
          if (short_of(bp + 7u)) { st = kStNeedInput; break; }  // (no code among the 7 bits at bp)
        }
        if (short_of(bp)) { st = kStNeedInput; break; }
        if (past_end()) { st = ZH_ERR_END_OF_BUFFER; break; }
        if (sym <= 15) {
          if (lane == 0) s_lens[i] = (uint8_t)sym;
          prev = sym;
          i++;
        } else if (sym == 16) {
          if (i == 0) { st = ZH_ERR_INVALID_BUFFER; break; }
          const uint32_t rep = take(2) + 3;
          if (short_of(bp)) { st = kStNeedInput; break; }
          if (i + rep > 320) { st = ZH_ERR_INVALID_BUFFER; break; }
          if (lane < rep) s_lens[i + lane] = (uint8_t)prev;
          i += rep;
        } else if (sym == 17 || sym == 18) {
          const uint32_t rep = sym == 17 ? take(3) + 3 : take(7) + 11;
          if (short_of(bp)) { st = kStNeedInput; break; }
          for (uint32_t j = lane; j < rep && i + j < 320 + 16; j += 64) s_lens[i + j] = 0;
          prev = 0;
          i += rep;
        } else {
          st = ZH_ERR_INVALID_SYMBOL;
          break;
        }
        if (i > total) { st = ZH_ERR_INVALID_BUFFER; break; }
      }
      if (st != ZH_OK) break;
    }
    {
      const uint32_t dist_at = btype == 1 ? 288u : hlit;
      st = build_table(s_lens, hlit, s_lit, kLitBits, 0, &s_tab_lit, s_val_lit, s_cnt, kLitSub);
      if (st != ZH_OK) break;
      st = build_table(s_lens + dist_at, hdist, s_dst, kDistBits, 1, &s_tab_dist, s_val_dist, s_cnt);
      if (st != ZH_OK) break;
    }

    for (;;) {  // inflate.nim:173-250, one round = up to 128 bit positions
      KPROF_MARK(1);
#ifndef ZH_EMU
      __builtin_amdgcn_s_setprio(1);
#endif
      ensure();
      KPROF_MARK(6);
      // ---- every lane decodes the tokens that would start at bits bp + lane (window A)
      // and bp + 64 + lane (window B): two independent dependency chains per lane; B is
      // used when A's chain runs into it cleanly and both together make at most 64 bytes ----
      const uint32_t wi = (uint32_t)((bp + lane) >> 5), sh = ((uint32_t)bp + lane) & 31u;
      // (the output wave's status travels with these reads: a round's delay in noticing a failure
      // costs nothing, the exposed LDS round trip of a read behind the barrier did)
      const int32_t ostatus = s_ostatus;
      const uint32_t d0 = s_in[wi & (kInWords - 1u)], d1 = s_in[(wi + 1u) & (kInWords - 1u)],
                     d2 = s_in[(wi + 2u) & (kInWords - 1u)], d3 = s_in[(wi + 3u) & (kInWords - 1u)],
                     d4 = s_in[(wi + 4u) & (kInWords - 1u)];
      struct Tok {
        uint32_t v_lo, v_hi, e, tbits, outlen, val;  // val: literal byte or match distance
        bool is_lit;
      };
      // `flag` in the lanes whose bit is set in the wave-uniform mask (one select on the mask
      // instead of a 64-bit shift per lane)
      auto lane_flag = [&](uint64_t mask, uint32_t flag) -> uint32_t {
#ifdef ZH_EMU
        return (mask >> lane) & 1ull ? flag : 0u;
#else
        uint32_t r;
        asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(r) : "v"(flag), "s"(mask));
        return r;
#endif
      };
      auto decode_tok = [&](uint32_t v_lo, uint32_t v_hi) -> Tok {
        Tok t;
        t.v_lo = v_lo;
        t.v_hi = v_hi;
        uint32_t e = s_lit[v_lo & ((1u << kLitBits) - 1u)];
        if (e & 0x400u) e = s_lit[(e >> 16) + ((v_lo >> kLitBits) & ((1u << (e & 15u)) - 1u))];  // a longer code
        const uint32_t L = e & 15u, eb = (e >> 4) & 15u;
        t.e = e;
        t.is_lit = (e & 0x8000u) != 0;
        const uint32_t lenval = (e >> 16) + ((v_lo >> L) & ((1u << eb) - 1u));
        // (32-bit funnel shifts: L + eb <= 20 and, with a distance code from the 8-bit table, o3 <= 28)
        const uint32_t o2 = L + eb;
        const uint32_t de = s_dst[zh_alignbit(v_hi, v_lo, o2) & ((1u << kDistBits) - 1u)];
        const uint32_t o3 = o2 + (de & 15u), deb = (de >> 4) & 15u;
        t.val = t.is_lit ? (e >> 16) & 0xffu : (de >> 16) + (zh_alignbit(v_hi, v_lo, o3) & ((1u << deb) - 1u));
        if (t.is_lit) t.tbits = L;  // bits of the whole token; 0x8000: not decodable here
        else if (e != 0 && ((e >> 8) & 3u) == kKindBase && de != 0 && ((de >> 8) & 3u) == kKindBase) t.tbits = o3 + deb;
        else t.tbits = 0x8000u;
        t.outlen = t.is_lit ? 1u : lenval;
        return t;
      };
      const Tok A = decode_tok(zh_alignbit(d1, d0, sh), zh_alignbit(d2, d1, sh));
      const Tok B = decode_tok(zh_alignbit(d3, d2, sh), zh_alignbit(d4, d3, sh));

      // ---- the chain of real token starts ----
      uint64_t chain = 0, chainB = 0;
      uint32_t pos = 0;
#ifdef ZH_KPROF
      asm volatile("" ::"v"(A.tbits), "v"(B.tbits));  // (timers: the decode is done here)
#endif
      KPROF_MARK(4);
#ifdef ZH_EMU
      while (pos < 64u) {
        const uint32_t tv = __builtin_amdgcn_readlane(A.tbits, pos);
        if (tv & 0x8000u) break;
        chain |= 1ull << pos;
        pos += tv;
      }
      const bool useB = pos >= 64u;
      if (useB) {
        while (pos < 128u) {
          const uint32_t tv = __builtin_amdgcn_readlane(B.tbits, pos - 64u);
          if (tv & 0x8000u) break;
          chainB |= 1ull << (pos - 64u);
          pos += tv;
        }
      }
#else
      // the same two loops, five instructions and one taken branch per symbol: a token that
      // cannot be decoded here has length 0x8000, which ends the loop like the end of the window
      // does; its lane's bit is taken back afterwards (lane select and s_bitset use pos[5:0])
      {
        uint32_t tv;
        asm volatile(
            "1:\n\t"
            "v_readlane_b32 %[tv], %[tb], %[pos]\n\t"
            "s_bitset1_b64 %[ch], %[pos]\n\t"
            "s_add_u32 %[pos], %[pos], %[tv]\n\t"
            "s_cmp_lt_u32 %[pos], 64\n\t"
            "s_cbranch_scc1 1b\n\t"
            "s_bitcmp0_b32 %[pos], 15\n\t"
            "s_cbranch_scc1 2f\n\t"
            "s_and_b32 %[pos], %[pos], 0x7fff\n\t"
            "s_bitset0_b64 %[ch], %[pos]\n\t"
            "2:"
            : [tv] "=&s"(tv), [pos] "+s"(pos), [ch] "+s"(chain)
            : [tb] "v"(A.tbits)
            : "scc");
      }
      const bool useB = pos >= 64u;  // (a chain that stopped in window A left pos below 64)
      if (useB) {
        uint32_t tv;
        asm volatile(
            "1:\n\t"
            "v_readlane_b32 %[tv], %[tb], %[pos]\n\t"
            "s_bitset1_b64 %[ch], %[pos]\n\t"
            "s_add_u32 %[pos], %[pos], %[tv]\n\t"
            "s_cmp_lt_u32 %[pos], 0x80\n\t"
            "s_cbranch_scc1 1b\n\t"
            "s_bitcmp0_b32 %[pos], 15\n\t"
            "s_cbranch_scc1 2f\n\t"
            "s_and_b32 %[pos], %[pos], 0x7fff\n\t"
            "s_bitset0_b64 %[ch], %[pos]\n\t"
            "2:"
            : [tv] "=&s"(tv), [pos] "+s"(pos), [ch] "+s"(chainB)
            : [tb] "v"(B.tbits)
            : "scc");
      }
#endif
      KPROF_MARK(5);
#ifndef ZH_EMU
      __builtin_amdgcn_s_setprio(0);
#endif
      bool cut = false;  // kResume: the end of the input lies inside the chain
      if constexpr (kResume) {
        // the tokens that the end of the input cuts, and all behind them, are not the output wave's: they leave the
        // chain, and the round is the stream's last
        const uint64_t nbits = end * 8;
        const uint64_t inA = __ballot(bp + lane + A.tbits <= nbits);
        const uint64_t inB = __ballot(bp + 64u + lane + B.tbits <= nbits);
        cut = (chain & ~inA) != 0 || (useB && (chainB & ~inB) != 0);
        chain &= inA;
        chainB &= inB;
      }
      // ---- hand the round over (the output wave works out the offsets) ----
      RoundDesc& d = s_desc[rk & 1u];
      d.rec[0][lane] = A.outlen | (A.is_lit ? 1u << 9 : 0u) | lane_flag(chain, 1u << 10) | (A.val << 16);
      if (useB)
        d.rec[1][lane] = B.outlen | (B.is_lit ? 1u << 9 : 0u) | lane_flag(chainB, 1u << 10) | (B.val << 16);
      bp += pos;
      bool block_done = false;
      uint32_t tail = kTailNone, tail_a = 0, tail_b = 0;
      if (kResume && cut) {
        st = lastf ? (int)ZH_ERR_END_OF_BUFFER : kStNeedInput;
      } else if (pos < 64u || (useB && pos < 128u)) {
        // ---- the token at bp stopped the chain: decode it alone (inflate.nim:67-102) ----
        // (the builtin returns int: widen through uint32_t, or the low word sign-extends)
        uint32_t sv_lo, sv_hi, se;
        if (pos < 64u) {
          sv_lo = __builtin_amdgcn_readlane(A.v_lo, pos);
          sv_hi = __builtin_amdgcn_readlane(A.v_hi, pos);
          se = __builtin_amdgcn_readlane(A.e, pos);
        } else {
          sv_lo = __builtin_amdgcn_readlane(B.v_lo, pos - 64u);
          sv_hi = __builtin_amdgcn_readlane(B.v_hi, pos - 64u);
          se = __builtin_amdgcn_readlane(B.e, pos - 64u);
        }
        uint64_t sv = (uint64_t)sv_lo | ((uint64_t)sv_hi << 32);
        uint32_t used;
        uint32_t nocode = 0;  // kResume: bits a pattern without a code counts as
        if (se == 0) {  // longer than the LUT, or unassigned
          uint32_t nb;
          const uint32_t sym = decode_symbol_slow<true>((uint32_t)sv, kLitBits, &s_tab_lit, s_val_lit, &nb);
          se = litlen_entry(sym, 0);
          used = nb;
          if (kResume && sym == 0xffffu) nocode = 15u;
        } else {
          used = se & 15u;
        }
        sv >>= used;
        const uint32_t kind = (se >> 8) & 3u;
        if (se & 0x8000u) {  // a literal with a long code
          tail = kTailLiteral;
          tail_a = (se >> 16) & 0xffu;
        } else if (kind == kKindEob) {
          block_done = true;
        } else if (kind == kKindBad) {  // inflate.nim:202-204
          st = ZH_ERR_INVALID_BUFFER;
        } else {
          const uint32_t seb = (se >> 4) & 15u;
          const uint32_t length = (se >> 16) + ((uint32_t)sv & ((1u << seb) - 1u));
          sv >>= seb;
          used += seb;
          uint32_t sde = zh_bcast(s_dst[(uint32_t)sv & ((1u << kDistBits) - 1u)]);
          uint32_t dnb;
          if (sde == 0) {
            const uint32_t dsym = decode_symbol_slow<true>((uint32_t)sv, kDistBits, &s_tab_dist, s_val_dist, &dnb);
            sde = dist_entry(dsym, 0);
            if (kResume && dsym == 0xffffu) nocode = 15u;
          } else {
            dnb = sde & 15u;
          }
          sv >>= dnb;
          used += dnb;
          if (((sde >> 8) & 3u) == kKindBad) {  // inflate.nim:211-213
            st = ZH_ERR_INVALID_BUFFER;
          } else {
            const uint32_t sdeb = (sde >> 4) & 15u;
            tail = kTailMatch;
            tail_a = length;
            tail_b = (sde >> 16) + ((uint32_t)sv & ((1u << sdeb) - 1u));
            used += sdeb;
          }
        }
        if (short_of(bp + used + nocode)) {  // the end of the input cuts the token: nothing of it counts
          st = kStNeedInput;
          tail = kTailNone;
          block_done = false;
        }
        bp += used;
      }
      // tokens decoded from beyond the end of the input are caught here at the latest
      if (st == ZH_OK && past_end()) st = ZH_ERR_END_OF_BUFFER;
      if (lane == 0) {
        d.use_b = useB ? 1u : 0u;
        d.tail = st == ZH_OK ? tail : kTailNone;
        d.tail_a = tail_a;
        d.tail_b = tail_b;
      }
      KPROF_MARK(1);
      __syncthreads();
      KPROF_MARK(0);
      KPROF_COUNT(2, 1);
      rk++;
      if (st == ZH_OK && ostatus != ZH_OK) st = ostatus;
      if (st != ZH_OK || block_done) break;
    }
  }
  if (kSeek && st == ZH_OK && bp != stop_at) st = ZH_ERR_INVALID_BUFFER;  // (a final block that ends elsewhere)
  if constexpr (kResume) {
    if (st == ZH_OK) send_tail(kTailMark, 1, 0, bp);  // behind the final block
  }
  send_tail(kTailEnd, (uint32_t)st, 0, 0);
  KPROF_COUNT(3, 1);
  KPROF_FLUSH(24, 8);
}
