// What the inflate kernels READ with, once: loads that stop at the stream's end, the canonical slow-symbol decode,
// the serial block-header reader and the wave-wide code-length walk (the tables they read into are
// zh_inflate_tables.h's).  These carry the reference's checks in the reference's order -- which check comes first
// decides the status a damaged stream gets -- so zh_inflate.hip, zh_inflate_split.hip and zh_inflate_seg.hip
// come here for them (the one exception is named at BlockHeaderReader).
#pragma once
#include "zh_inflate_tables.h"

namespace {

// ---- loads that read zero behind the stream's end ----
// the dword at byte offset `off` (a multiple of four) of the dword-aligned `asrc`; `end`: first byte offset past the stream
__device__ __forceinline__ uint32_t load_dword_end(const uint32_t* asrc, uint64_t off, uint64_t end) {
  if (off >= end) return 0u;
  uint32_t v = asrc[off >> 2];
  if (off + 4 > end) v &= (1u << (8 * (uint32_t)(end - off))) - 1u;
  return v;
}
// the little-endian T at byte b (any alignment) of the `len` bytes at src
template <typename T>
__device__ __forceinline__ T load_le_end(const uint8_t* src, uint64_t len, uint64_t b) {
  T v = 0;
  if (b + sizeof(T) <= len) {
    struct __attribute__((packed)) U { T v; };
    v = reinterpret_cast<const U*>(src + b)->v;
  } else {
    for (uint32_t i = 0; i < sizeof(T); i++)
      if (b + i < len) v |= (T)src[b + i] << (8 * i);
  }
  return v;
}
// the 32 bits at bit `at` of staged dwords
__device__ __forceinline__ uint32_t bits_at(const uint32_t* words, uint32_t at) {
  return zh_alignbit(words[(at >> 5) + 1u], words[at >> 5], at);
}

// inflate.nim:67-91 decodeSymbolSlow for codes longer than the LUT on the bits in `bits`: returns the symbol
// (0xffff = unassigned code) and its length in *nb (0 then).  kUniform: the caller runs wave-uniform, and the LDS
// reads stay on scalar registers.
template <bool kUniform>
__device__ __forceinline__ uint32_t decode_symbol_slow(uint32_t bits, uint32_t lut_bits, const HuffTab* tab,
                                                       const uint16_t* values, uint32_t* nb) {
  auto rd = [](uint32_t v) -> uint32_t { return kUniform ? zh_bcast(v) : v; };
  const uint32_t k = __brev(bits) >> 16;
  uint32_t cl = lut_bits + 1;
  while (cl < 16 && k >= rd(tab->max_codes[cl])) cl++;
  *nb = 0;
  if (cl >= 16) return 0xffffu;
  const uint32_t id = ((k >> (16 - cl)) - rd(tab->first_code[cl]) + rd(tab->first_symbol[cl])) & 0xffffu;
  *nb = cl;
  return rd(values[id]);
}

// ---------------------------------------------------------------------------
// The block header (inflate.nim:252-289 and 111-171) read by ONE WAVE, wave-uniform: wave 0 of
// zh_inflate_tokens_kernel.  (zh_inflate_kernel's decode wave keeps a copy of fields() and code_lengths() in its
// block loop: with this reader it measured 3 % slower on the indexed form.  A change here goes there too.)
// `fetch(at)`: the 64 stream bits at bit `at`, out of the staged header; `bp`: the caller's bit position, in fetch's
// coordinates, which the reader moves; `base`: the stream bit (from the dword-aligned base) of fetch's bit 0, a
// multiple of 32; `end`: the first byte offset past the stream.  fields() leaves bp behind the fixed fields (a
// stored block: at its first raw byte), code_lengths() behind the header.
// ---------------------------------------------------------------------------
template <typename Fetch>
struct BlockHeaderReader {
  Fetch fetch;
  uint64_t& bp;
  const uint64_t base, end;
  uint64_t hb = 0;  // the bits at bp, hc of them
  uint32_t hc = 0;
  uint32_t bfinal = 0, btype = 0, hlit = 288, hdist = 30, hclen = 0, stored_len = 0;

  __device__ __forceinline__ BlockHeaderReader(Fetch f, uint64_t& bp_, uint64_t base_, uint64_t end_)
      : fetch(f), bp(bp_), base(base_), end(end_) {}
  __device__ __forceinline__ void need() {
    if (hc < 32u) {
      hb = fetch(bp);
      hc = 64;
    }
  }
  __device__ __forceinline__ uint32_t take(uint32_t nbits) {  // nbits <= 16, after need()
    const uint32_t v = (uint32_t)hb & ((1u << nbits) - 1u);
    hb >>= nbits;
    hc -= nbits;
    bp += nbits;
    return v;
  }
  __device__ __forceinline__ bool past_end() const { return base + bp > end * 8; }  // the role of `bitsBuffered < 0`

  // BFINAL, BTYPE and what follows them at bp: a stored block's LEN / NLEN, a dynamic block's HLIT / HDIST / HCLEN
  __device__ __forceinline__ int fields() {
    hc = 0;
    need();
    bfinal = take(1);
    btype = take(2);
    if (btype == 0) {  // inflate.nim:252-266 inflateNoCompression
      bp = (bp + 7u) & ~(uint64_t)7;
      hc = 0;
      need();
      stored_len = take(16);
      if (stored_len + take(16) != 65535u) return ZH_ERR_INVALID_BUFFER;
      if (((base + bp) >> 3) + stored_len > end) return ZH_ERR_END_OF_BUFFER;
    } else if (btype == 3) {
      return ZH_ERR_BLOCK_HEADER;
    } else if (btype == 2) {  // inflate.nim:115-120
      hlit = take(5) + 257;
      hdist = take(5) + 1;
      hclen = take(4) + 4;
      if (hlit > 286 || hdist > 30) return ZH_ERR_INVALID_BUFFER;
    } else {
      hlit = 288;
      hdist = 30;
    }
    return ZH_OK;
  }

  // The code lengths of a fixed or dynamic block into lens[0 .. hlit + hdist) (fixed: the distance code's at 288),
  // the dynamic header's one symbol after the other with every check of inflate.nim:121-171 in its order.
  // cl_lut (128 entries), tab_cl, val_cl, cnt: LDS for the code-length code's table.
  __device__ __forceinline__ int code_lengths(uint8_t* lens, uint32_t* cl_lut, HuffTab* tab_cl, uint16_t* val_cl, uint32_t* cnt) {
    const unsigned lane = zh_lane();
    zh_wave_sync();
    if (btype == 1) {  // fixed codes, inflate.nim:111-113 (rebuilt per block like the reference)
      for (uint32_t s = lane; s < 288; s += 64) lens[s] = (uint8_t)(s <= 143 ? 8 : s <= 255 ? 9 : s <= 279 ? 7 : 8);
      if (lane < 30) lens[288 + lane] = 5;
      return ZH_OK;
    }
    if (lane < 20) lens[lane] = 0;
    zh_wave_sync();
    for (uint32_t i = 0; i < hclen; i++) {
      need();
      const uint32_t v = take(3);
      if (lane == 0) lens[c_clcl_order[i]] = (uint8_t)v;
    }
    const int st = build_table(lens, 19, cl_lut, 7, 2, tab_cl, val_cl, cnt);
    if (st != ZH_OK) return st;
    const uint32_t total = hlit + hdist;
    uint32_t i = 0, prev = 0;
    while (i != total) {
      need();
      uint32_t sym;
      const uint32_t e = zh_bcast(cl_lut[(uint32_t)hb & 127u]);
      if (e) {
        take(e & 15u);
        sym = e >> 16;
      } else {
        uint32_t nb;
        sym = decode_symbol_slow<true>((uint32_t)hb, 7, tab_cl, val_cl, &nb);
        take(nb);
      }
      if (past_end()) return ZH_ERR_END_OF_BUFFER;
      if (sym <= 15) {
        if (lane == 0) lens[i] = (uint8_t)sym;
        prev = sym;
        i++;
      } else if (sym == 16) {
        if (i == 0) return ZH_ERR_INVALID_BUFFER;
        const uint32_t rep = take(2) + 3;
        if (i + rep > 320) return ZH_ERR_INVALID_BUFFER;
        if (lane < rep) lens[i + lane] = (uint8_t)prev;
        i += rep;
      } else if (sym == 17 || sym == 18) {
        const uint32_t rep = sym == 17 ? take(3) + 3 : take(7) + 11;
        for (uint32_t j = lane; j < rep && i + j < 320 + 16; j += 64) lens[i + j] = 0;
        prev = 0;
        i += rep;
      } else {
        return ZH_ERR_INVALID_SYMBOL;
      }
      if (i > total) return ZH_ERR_INVALID_BUFFER;
    }
    return ZH_OK;
  }
};

// ---------------------------------------------------------------------------
// The code lengths of a dynamic header (inflate.nim:115-171) by ONE WAVE instead of one lane's scalar chain:
// the 64 lanes decode the code-length symbols that start at 64 consecutive bit positions, a wave-uniform walk
// (one v_readlane a symbol) picks the ones really in the sequence, repeat counts become places by a prefix sum.
// `hdr`: the header staged in LDS (dwords), bit 0 of hdr[0] = bit 0 of the staged range; `q`: the first bit
// behind HCLEN; `end_bits`: the input's end in the same bit coordinates; `lut8`: 128 bytes of LDS.
// Every window, all lanes call sink(at, rep, val, mine): lane `mine` holds `rep` lengths `val` from index `at`
// (sums over the wave are the sink's to take; false from it ends the walk).  Returns the bit behind the last
// symbol -- or 0 where the header is anything but clean: a code-length code that is over-subscribed or has no
// code for a position ON the sequence (nb = 64 there: a position the walk does not come by may read as anything),
// a repeat with nothing before it or past the end, input that ends inside.  The tokens kernel then runs the serial
// reader, which knows the reference's status for every such case; the segment search only ever asks about
// complete code-length codes (seg_precode_complete), where no position is without a code, and takes 0 as "no".
// ---------------------------------------------------------------------------
template <typename Sink>
__device__ __forceinline__ uint32_t code_lengths_walk(const uint32_t* hdr, uint32_t q, uint32_t hlit, uint32_t hdist,
                                                      uint32_t hclen, uint64_t end_bits, uint8_t* lut8, Sink sink) {
  const unsigned lane = zh_lane();
  // lane s < 19: the length of code-length symbol s; its place in the header is the inverse of c_clcl_order
  // {3, 17, 15, 13, 11, 9, 7, 5, 4, 6, 8, 10, 12, 14, 16, 18, 0, 1, 2}, five bits a symbol in two constants
  constexpr uint64_t kPlaceLo = 3ull | 17ull << 5 | 15ull << 10 | 13ull << 15 | 11ull << 20 | 9ull << 25 | 7ull << 30 |
                                5ull << 35 | 4ull << 40 | 6ull << 45 | 8ull << 50 | 10ull << 55;
  constexpr uint64_t kPlaceHi = 12ull | 14ull << 5 | 16ull << 10 | 18ull << 15 | 0ull << 20 | 1ull << 25 | 2ull << 30;
  const uint32_t place = lane < 12u ? (uint32_t)(kPlaceLo >> (5u * lane)) & 31u
                                    : lane < 19u ? (uint32_t)(kPlaceHi >> (5u * (lane - 12u))) & 31u : 99u;
  const uint32_t l = place < hclen ? bits_at(hdr, q + 3u * place) & 7u : 0u;
  q += 3u * hclen;
  // canonical codes (inflate.nim:29-65): symbols of one length in symbol order
  uint32_t code = 0, next = 0;
#pragma unroll
  for (uint32_t k = 1; k <= 7; k++) {
    const uint64_t m = __ballot(l == k);
    if (l == k) code = next + (uint32_t)__popcll(m & zh_lanemask_lt());
    next = (next + (uint32_t)__popcll(m)) << 1;
  }
  if (next > 256u) return 0;  // over-subscribed: `next` has come to twice the Kraft sum in 1/128ths
  zh_wave_sync();  // (whoever used the table before has read it)
  if (lane < 32u) reinterpret_cast<uint32_t*>(lut8)[lane] = 0;
  zh_wave_sync();
  if (l) {
    const uint32_t rev = __brev(code) >> (32u - l);  // the stream carries codes first bit first
    for (uint32_t e = rev; e < 128u; e += 1u << l) lut8[e] = (uint8_t)(lane | (l << 5));
  }
  zh_wave_sync();
  const uint32_t total = hlit + hdist;
  uint32_t i = 0, prev = 0;
  while (i < total) {
    const uint32_t w = bits_at(hdr, q + lane);  // the symbol that starts at bit q + lane
    const uint32_t e = lut8[w & 127u], sym = e & 31u, cl = e >> 5;
    const uint32_t x = w >> cl;
    uint32_t rep = 1, val = sym, nb = cl;
    if (sym == 16u) {
      rep = (x & 3u) + 3u;
      nb += 2u;
    } else if (sym == 17u) {
      rep = (x & 7u) + 3u;
      nb += 3u;
      val = 0;
    } else if (sym == 18u) {
      rep = (x & 127u) + 11u;
      nb += 7u;
      val = 0;
    }
    if (cl == 0u) nb = 64u;  // no code here: a walk that comes by ends the fast path
    // the walk: which of the 64 positions start a symbol of the sequence
    uint64_t on = 0;
    uint32_t pos = 0;
    while (pos < 64u) {
      on |= 1ull << pos;
      pos += (uint32_t)__builtin_amdgcn_readlane((int)nb, (int)pos);
    }
    bool mine = (on >> lane) & 1ull;
    const uint32_t incl = zh_wave_scan(mine ? rep : 0u);
    const uint32_t at = i + incl - (mine ? rep : 0u);  // index of my first entry
    if (mine && at >= total) mine = false;             // behind the last length: not part of the header
    const uint64_t ON = __ballot(mine);                // (bit 0 is set: at = i < total)
    if (__ballot(mine && (cl == 0u || at + rep > total))) return 0;  // inflate.nim:161-162: runs past the end
    if (i == 0 && (uint32_t)__builtin_amdgcn_readlane((int)sym, 0) == 16u) return 0;  // nothing to repeat
    // "previous length" for symbol 16: the nearest symbol before that is not a 16 (17 / 18 leave zero)
    const uint64_t plain = __ballot(mine && sym != 16u) & zh_lanemask_lt();
    const uint32_t from = plain ? 63u - (uint32_t)__clzll((long long)plain) : 0u;
    const uint32_t pv = (uint32_t)__shfl((int)val, (int)from, 64);
    if (sym == 16u) val = plain ? pv : prev;
    if (!sink(at, rep, val, mine)) return 0;
    const uint32_t lastl = 63u - (uint32_t)__clzll((long long)ON);  // behind the last symbol taken
    i = (uint32_t)__builtin_amdgcn_readlane((int)(at + rep), (int)lastl);
    prev = (uint32_t)__builtin_amdgcn_readlane((int)val, (int)lastl);
    q += lastl + (uint32_t)__builtin_amdgcn_readlane((int)nb, (int)lastl);
  }
  if ((uint64_t)q > end_bits) return 0;
  return q;
}

// The walk that fills lens[0 .. hlit + hdist) for the tokens kernel (out of line: that kernel's register budget).
__device__ __noinline__ uint32_t code_lengths_wave(const uint32_t* hdr, uint32_t q, uint32_t hlit, uint32_t hdist, uint32_t hclen,
                                      uint64_t end_bits, uint8_t* lens, uint8_t* lut8) {
  zh_wave_sync();
  for (uint32_t i = zh_lane(); i < (320u + 16u) / 4u; i += 64u) reinterpret_cast<uint32_t*>(lens)[i] = 0;
  const uint32_t r = code_lengths_walk(hdr, q, hlit, hdist, hclen, end_bits, lut8,
                                       [&](uint32_t at, uint32_t rep, uint32_t val, bool mine) -> bool {
    if (mine && val)  // (zeros are there already; what is left repeats six times at most)
      for (uint32_t j = 0; j < rep; j++) lens[at + j] = (uint8_t)val;
    return true;
  });
  zh_wave_sync();
  return r;
}

}  // namespace
