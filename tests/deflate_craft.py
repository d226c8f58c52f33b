"""A deflate stream builder for tests, written from RFC 1951: an LSB-first bit writer with stored, fixed and dynamic
blocks whose every field a test can dictate -- code lengths (incomplete and over-subscribed sets included), HCLEN, the
code-length code and the exact sequence of 0-15 / 16 / 17 / 18 symbols, any length / distance pair, bit patterns that
are no code at all.  The expected plaintext is kept by construction (a literal appends a byte, a match copies byte by
byte, a stored block appends its data): it comes from no decoder.  A stream that is meant to fail records None and the
status its single fault must give.  The bit positions of every token and block header are recorded, so a test can
assert which bit phases it covered.  read_blocks is the way back for sound streams: block types, the headers' code
lengths and the tokens, as an encoder wrote them."""

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LIT_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8   # 288 symbols: 286 and 287 have codes and no meaning
FIXED_DIST_LENS = [5] * 32                                    # 32 patterns: 30 and 31 have no meaning

# the statuses a malformed stream gives (the reference's messages, numbered as the library numbers them)
INVALID_BUFFER, END_OF_BUFFER, BLOCK_HEADER, INVALID_SYMBOL = 13, 15, 17, 18


def canonical_codes(lens):
    """RFC 1951 3.2.2: codes (MSB first) from code lengths; also for incomplete sets.  An over-subscribed set gets
    codes that overflow their length -- such a block is refused at its header, nobody decodes with them."""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    code, next_code = 0, [0] * 17
    for bits in range(1, 17):
        code = (code + count[bits - 1]) << 1
        next_code[bits] = code
    out = []
    for n in lens:
        if n:
            out.append(next_code[n])
            next_code[n] += 1
        else:
            out.append(None)
    return out


def kraft(lens):
    """sum of 2^-len as a fraction of 2^15: 32768 is a complete set"""
    return sum(1 << (15 - n) for n in lens if n)


def rle_plain(lens):
    """code lengths as code-length symbols without any repeat symbol"""
    return [(n, 0) for n in lens]


def rle_zero_runs(lens):
    """code lengths as code-length symbols, runs of zeros as 17 / 18, nothing else repeated"""
    out, i = [], 0
    while i < len(lens):
        j = i
        while j < len(lens) and lens[j] == 0:
            j += 1
        run = j - i
        while run >= 3:
            take = min(run, 138)
            out.append((17, take - 3) if take <= 10 else (18, take - 11))
            run -= take
            i += take
        while i < j:
            out.append((0, 0))
            i += 1
        if i < len(lens):
            out.append((lens[i], 0))
            i += 1
    return out


def expand_cl_symbols(symbols):
    """what a reader makes of a code-length symbol sequence (RFC 1951 3.2.7); None where 16 comes first"""
    out = []
    for sym, extra in symbols:
        if sym <= 15:
            out.append(sym)
        elif sym == 16:
            if not out:
                return None
            out += [out[-1]] * (3 + extra)
        elif sym == 17:
            out += [0] * (3 + extra)
        else:
            out += [0] * (11 + extra)
    return out


def complete_cl_lens(used):
    """lengths of a complete code-length code over the symbols `used` (at least two, so that zlib takes it)"""
    used = sorted(set(used))
    if len(used) == 1:
        used = sorted(set(used) | {0 if used[0] != 0 else 1})
    k = (len(used) - 1).bit_length()
    short = (1 << k) - len(used)  # that many symbols one bit shorter
    lens = [0] * 19
    for j, s in enumerate(used):
        lens[s] = k - 1 if j < short else k
    assert kraft(lens) == 32768 and max(lens) <= 7
    return lens


_FIXED_CODES = (canonical_codes(FIXED_LIT_LENS), canonical_codes(FIXED_DIST_LENS))


class Stream:
    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.nacc = 0
        self.out = bytearray()        # the expected plaintext while the stream is sound
        self.status = None            # the status of the fault once one is planted
        self.tokens = []              # (bit position, bits, kind) of every literal / match / end-of-block
        self.headers = []             # (bit position, BTYPE) of every block header
        self.final_pad = 0            # what the bits behind the last block, up to the byte boundary, hold
        self.lit_codes = self.lit_lens = self.dist_codes = self.dist_lens = None

    # ---- bits ----
    @property
    def bitpos(self):
        return len(self.buf) * 8 + self.nacc

    def raw_bits(self, v, n):
        """n bits of v, least significant first (header fields, extra bits)"""
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.nacc
        self.nacc += n
        while self.nacc >= 8:
            self.buf.append(self.acc & 0xff)
            self.acc >>= 8
            self.nacc -= 8

    def _code(self, code, nbits):
        rev = int(format(code, "0%db" % nbits)[::-1], 2) if nbits else 0
        self.raw_bits(rev, nbits)

    def raw_code(self, alphabet, bits, nbits):
        """a bit pattern written the way a Huffman code is (first bit of `bits` = its most significant) that need not
        be a code of `alphabet` ('lit' / 'dist' / 'cl': only recorded)"""
        self.tokens.append((self.bitpos, nbits, "raw-" + alphabet))
        self._code(bits, nbits)

    def align(self, fill=0):
        n = (8 - self.nacc) % 8
        self.raw_bits(fill & ((1 << n) - 1), n)

    def append_bytes(self, blob, plain):
        """a byte-aligned-ending deflate fragment made elsewhere (an encoder's blocks), at the current bit position"""
        for b in blob:
            self.raw_bits(b, 8)
        self.out += plain

    def expect_fail(self, status):
        if self.status is None:
            self.status = status

    # ---- blocks ----
    def _header(self, final, btype):
        self.headers.append((self.bitpos, btype))
        self.raw_bits(1 if final else 0, 1)
        self.raw_bits(btype, 2)

    def stored(self, data, final, pad_bits=0):
        """pad_bits: what the skipped bits up to the byte boundary hold"""
        assert len(data) <= 65535
        self._header(final, 0)
        self.align(pad_bits)
        self.raw_bits(len(data), 16)
        self.raw_bits(len(data) ^ 0xffff, 16)
        self.buf += data
        self.out += data

    def fixed_block(self, final):
        self._header(final, 1)
        self.lit_lens, self.dist_lens = FIXED_LIT_LENS, FIXED_DIST_LENS
        self.lit_codes, self.dist_codes = _FIXED_CODES

    def dynamic_block(self, lit_lens, dist_lens, final, cl_plan=None):
        """HLIT = len(lit_lens), HDIST = len(dist_lens) (the 5-bit fields wrap like the format's: 287 / 288 and
        31 / 32 can be written).  cl_plan: {'symbols': [(0-18, extra bits' value)], 'cl_lens': 19 lengths,
        'hclen': 4..19, 'check': False where the symbols are not meant to spell the lengths}"""
        plan = dict(cl_plan or {})
        symbols = plan.get("symbols")
        if symbols is None:
            symbols = rle_zero_runs(list(lit_lens) + list(dist_lens))
        if plan.get("check", True):
            assert expand_cl_symbols(symbols) == list(lit_lens) + list(dist_lens), "the plan does not spell the lengths"
        cl_lens = plan.get("cl_lens") or complete_cl_lens([s for s, _ in symbols])
        hclen = plan.get("hclen")
        if hclen is None:
            hclen = max([4] + [k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]])
        assert 4 <= hclen <= 19 and all(cl_lens[CL_ORDER[k]] == 0 for k in range(hclen, 19))
        assert 257 <= len(lit_lens) <= 288 and 1 <= len(dist_lens) <= 32
        self._header(final, 2)
        self.raw_bits(len(lit_lens) - 257, 5)
        self.raw_bits(len(dist_lens) - 1, 5)
        self.raw_bits(hclen - 4, 4)
        for k in range(hclen):
            self.raw_bits(cl_lens[CL_ORDER[k]], 3)
        cl_codes = canonical_codes(cl_lens)
        for sym, extra in symbols:
            if isinstance(sym, tuple):       # ('raw', bits, nbits): a pattern that is no code
                self._code(sym[1], sym[2])
                continue
            assert cl_lens[sym], "code-length symbol %d has no code" % sym
            self._code(cl_codes[sym], cl_lens[sym])
            if sym >= 16:
                self.raw_bits(extra, (2, 3, 7)[sym - 16])
        self.lit_lens, self.dist_lens = list(lit_lens), list(dist_lens)
        self.lit_codes, self.dist_codes = canonical_codes(lit_lens), canonical_codes(dist_lens)

    # ---- tokens ----
    def lit(self, b):
        self.tokens.append((self.bitpos, self.lit_lens[b], "lit"))
        self._code(self.lit_codes[b], self.lit_lens[b])
        self.out.append(b)

    def eob(self):
        self.tokens.append((self.bitpos, self.lit_lens[256], "eob"))
        self._code(self.lit_codes[256], self.lit_lens[256])

    def match(self, length, dist, length_symbol=None):
        """length_symbol: another symbol than the canonical one (284 with all five extra bits set is length 258)"""
        if length_symbol is None:
            length_symbol = 285 if length == 258 else 257 + max(k for k in range(28) if LEN_BASE[k] <= length)
        k = length_symbol - 257
        extra = length - LEN_BASE[k]
        assert 0 <= extra < (1 << LEN_EXTRA[k])
        d = max(j for j in range(30) if DIST_BASE[j] <= dist)
        start = self.bitpos
        self._code(self.lit_codes[length_symbol], self.lit_lens[length_symbol])
        self.raw_bits(extra, LEN_EXTRA[k])
        self._code(self.dist_codes[d], self.dist_lens[d])
        self.raw_bits(dist - DIST_BASE[d], DIST_EXTRA[d])
        self.tokens.append((start, self.bitpos - start, "match"))
        if dist > len(self.out):
            self.expect_fail(INVALID_BUFFER)  # (a distance beyond the start of the output)
        if self.status is None:
            at = len(self.out) - dist
            for i in range(length):
                self.out.append(self.out[at + i])

    # ---- results ----
    def cut_at_bit(self, bit):
        """the stream ends inside the field that holds `bit`: bits from there on are gone (the rest of that byte zero)"""
        self.align()
        del self.buf[(bit + 7) // 8:]
        if bit % 8:
            self.buf[-1] &= (1 << (bit % 8)) - 1

    def finish(self):
        """-> (raw deflate, plain or None, status or None)"""
        self.align(self.final_pad)
        if self.status is not None:
            return bytes(self.buf), None, self.status
        return bytes(self.buf), bytes(self.out), None


# ---- a reader, for the streams an encoder wrote ----
def _decode_table(lens):
    """{(length, code read first bit first): symbol} of a canonical code"""
    return {(n, c): s for s, (n, c) in enumerate(zip(lens, canonical_codes(lens))) if n}


def read_blocks(raw):
    """A plain RFC 1951 reader of a sound stream -> one dict a block: 'type' (0 stored, 1 fixed, 2 dynamic), 'final',
    'lit_lens' / 'dist_lens' (the header's code lengths, HLIT / HDIST entries; the fixed code's for type 1; None for
    type 0) and 'tokens': ('lit', byte) / ('match', length, distance) in order, a stored block's bytes as literals.
    The end-of-block symbol is no token.  Bits behind the final block up to the byte boundary are not looked at."""
    pos = 0

    def bits(n):
        nonlocal pos
        v = 0
        for i in range(n):
            v |= (raw[pos >> 3] >> (pos & 7) & 1) << i
            pos += 1
        return v

    def symbol(table):
        code = n = 0
        while True:
            code = code << 1 | bits(1)
            n += 1
            assert n <= 15, "no such code"
            if (n, code) in table:
                return table[(n, code)]

    out = []
    while True:
        final, btype = bits(1), bits(2)
        assert btype != 3
        blk = {"type": btype, "final": bool(final), "lit_lens": None, "dist_lens": None, "tokens": []}
        out.append(blk)
        if btype == 0:
            pos = (pos + 7) & ~7
            n, nn = bits(16), bits(16)
            assert n ^ nn == 0xffff
            blk["tokens"] = [("lit", b) for b in raw[pos >> 3:(pos >> 3) + n]]
            assert len(blk["tokens"]) == n
            pos += 8 * n
        else:
            if btype == 1:
                lit_lens, dist_lens = list(FIXED_LIT_LENS), list(FIXED_DIST_LENS)
            else:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl_lens = [0] * 19
                for k in range(hclen):
                    cl_lens[CL_ORDER[k]] = bits(3)
                cl, lens = _decode_table(cl_lens), []
                while len(lens) < hlit + hdist:
                    s = symbol(cl)
                    if s <= 15:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits(2))
                    else:
                        lens += [0] * (3 + bits(3) if s == 17 else 11 + bits(7))
                assert len(lens) == hlit + hdist
                lit_lens, dist_lens = lens[:hlit], lens[hlit:]
            blk["lit_lens"], blk["dist_lens"] = lit_lens, dist_lens
            lit, dist = _decode_table(lit_lens), _decode_table(dist_lens)
            while True:
                s = symbol(lit)
                if s < 256:
                    blk["tokens"].append(("lit", s))
                elif s == 256:
                    break
                else:
                    assert s <= 285
                    length = LEN_BASE[s - 257] + bits(LEN_EXTRA[s - 257])
                    d = symbol(dist)
                    assert d <= 29
                    blk["tokens"].append(("match", length, DIST_BASE[d] + bits(DIST_EXTRA[d])))
        if final:
            assert (pos + 7) >> 3 == len(raw), "bytes behind the final block"
            return out


def replay(blocks):
    """the plaintext of read_blocks' tokens"""
    out = bytearray()
    for blk in blocks:
        for t in blk["tokens"]:
            if t[0] == "lit":
                out.append(t[1])
            else:
                assert 1 <= t[2] <= len(out)
                for _ in range(t[1]):
                    out.append(out[-t[2]])
    return bytes(out)
