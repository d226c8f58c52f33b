"""A model of the resumable uncompress (include/zippy_hip.h: zh_uncompress_resume_batch) in plain Python, written from
RFC 1951 and the header's prose: one call of one stream -- step() -- with the state blob, the container's header and
trailer, and a decode loop of its own that keeps the blocks it completed when the input or the budget gives out.  No
engine and no zlib in here (the running CRC-32 and Adler-32 are written out below): tests/test_resume_model.py holds
it against zlib.decompressobj and against tests/seek_model.py.

The loop knows two ways to read.  Without `last`, nothing is decided by a bit at or beyond the end of the input: a
field, a code or a token that the end cuts is NEED_INPUT, and a pattern that no code claims is an error only with 7
(the code-length code) or 15 bits in hand.  With `last` the input reads as zeros behind its end and the checks are the
whole call's, in its order: an error of the token itself first, then the end of the input inside the token
(ZH_ERR_END_OF_BUFFER), then a distance beyond the window, then the budget."""
import bisect
import struct

from deflate_craft import CL_ORDER, DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA
from seek_model import Fail, _table

WINDOW = 32768
MAGIC = b"ZHRESUM1"
DF_DETECT, DF_ZLIB, DF_GZIP, DF_DEFLATE = 0, 1, 2, 3
DONE, NEED_INPUT, NEED_OUTPUT = 0, 1, 2
(OK, INVALID_FORMAT, DETECT, UNSUPPORTED_METHOD, COMPRESSION_INFO, INVALID_HEADER, PRESET_DICT, CHECKSUM, SIZE, GZIP_ID,
 RESERVED_FLAGS, UNSUPPORTED_FLAGS, INVALID_BUFFER) = 0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13
END_OF_BUFFER, BLOCK_HEADER, INVALID_SYMBOL, ARGUMENT = 15, 17, 18, 22
STATE = struct.Struct("<8sIIIIQQII16s")
assert STATE.size == 64


# ---- checksums, continued from a running value ----
def _crc_table():
    t = []
    for n in range(256):
        c = n
        for _ in range(8):
            c = (c >> 1) ^ 0xedb88320 if c & 1 else c >> 1
        t.append(c)
    return t


_CRC = _crc_table()


def crc32(data, crc=0):
    c = crc ^ 0xffffffff
    for b in data:
        c = _CRC[(c ^ b) & 255] ^ (c >> 8)
    return c ^ 0xffffffff


def adler32(data, adler=1):
    s1, s2 = adler & 0xffff, adler >> 16
    for o in range(0, len(data), 3800):
        for b in data[o:o + 3800]:
            s1 += b
            s2 += s1
        s1 %= 65521
        s2 %= 65521
    return s2 << 16 | s1


# ---- the state ----
def pack_state(fmt, phase, bit_skip, total_in, total_out, check, window, magic=MAGIC, version=1, win_len=None,
               reserved=bytes(16)):
    return STATE.pack(magic, version, fmt, phase, bit_skip, total_in, total_out, check,
                      len(window) if win_len is None else win_len, reserved) + bytes(window)


class State:
    """a state taken apart (no checks: the tests damage states through this as well)"""

    def __init__(self, blob):
        (self.magic, self.version, self.fmt, self.phase, self.bit_skip, self.total_in, self.total_out, self.check,
         self.win_len, self.reserved) = STATE.unpack_from(blob, 0)
        self.window = bytes(blob[64:])

    def pack(self):
        return pack_state(self.fmt, self.phase, self.bit_skip, self.total_in, self.total_out, self.check, self.window,
                          self.magic, self.version, self.win_len, self.reserved)


def sound(blob):
    """the header's rules for a state that can be right, in the order of its prose"""
    if len(blob) < 64:
        return False
    s = State(blob)
    return (s.magic == MAGIC and s.version == 1 and s.fmt in (DF_ZLIB, DF_GZIP, DF_DEFLATE) and s.phase in (1, 2)
            and s.bit_skip <= 7 and (s.phase == 1 or s.bit_skip == 0) and s.win_len == min(s.total_out, WINDOW)
            and len(blob) == 64 + s.win_len and s.reserved == bytes(16))


# ---- the container ----
def read_head(data, fmt, whole):
    """-> (status, need more input, resolved format, header length).  whole: the input is the whole stream and the
    length rules are zh_uncompress_batch's; otherwise every check waits until the bytes it reads are there: four for
    the detection, ten and the name, comment and header CRC for a gzip member, two for a zlib stream."""
    n = len(data)
    if fmt == DF_DETECT:
        if not whole and n < 4:
            return OK, True, 0, 0
        if (not whole or n > 18) and n >= 4 and data[0] == 31 and data[1] == 139 and data[2] == 8 and not data[3] & 0xe0:
            fmt = DF_GZIP
        elif ((not whole or n > 6) and n >= 2 and data[0] & 15 == 8 and data[0] >> 4 <= 7
              and (data[0] * 256 + data[1]) % 31 == 0):
            fmt = DF_ZLIB
        else:
            return DETECT, False, 0, 0
    short = (INVALID_BUFFER, False, fmt, 0) if whole else (OK, True, fmt, 0)
    if fmt == DF_GZIP:
        if n < (18 if whole else 10):
            return short
        flg = data[3]
        if data[0] != 31 or data[1] != 139:
            return GZIP_ID, False, fmt, 0
        if data[2] != 8:
            return UNSUPPORTED_METHOD, False, fmt, 0
        if flg & 0xe0:
            return RESERVED_FLAGS, False, fmt, 0
        if flg & 4:
            return UNSUPPORTED_FLAGS, False, fmt, 0
        p = 10
        for flag in (8, 16):
            if flg & flag:
                p = data.find(0, p)
                if p < 0:
                    return short
                p += 1
        if flg & 2:
            if p + 2 >= n if whole else p + 2 > n:
                return short
            p += 2
        if whole and p + 8 >= n:
            return short
        return OK, False, fmt, p
    if fmt == DF_ZLIB:
        if n < (6 if whole else 2):
            return short
        if data[0] & 15 != 8:
            return UNSUPPORTED_METHOD, False, fmt, 0
        if data[0] >> 4 > 7:
            return COMPRESSION_INFO, False, fmt, 0
        if (data[0] * 256 + data[1]) % 31:
            return INVALID_HEADER, False, fmt, 0
        if data[1] & 0x20:
            return PRESET_DICT, False, fmt, 0
        return OK, False, fmt, 2
    return (OK, False, fmt, 0) if fmt == DF_DEFLATE else (INVALID_FORMAT, False, fmt, 0)


def trailer_bytes(fmt):
    return 8 if fmt == DF_GZIP else 4 if fmt == DF_ZLIB else 0


def check_trailer(t, fmt, check, total_out):
    if fmt == DF_GZIP:
        if struct.unpack_from("<I", t, 0)[0] != check:
            return CHECKSUM
        if struct.unpack_from("<I", t, 4)[0] != total_out & 0xffffffff:
            return SIZE
    elif fmt == DF_ZLIB and struct.unpack_from(">I", t, 0)[0] != check:
        return CHECKSUM
    return OK


# ---- the decode loop ----
class _Stop(Exception):
    def __init__(self, why, status=OK):
        self.why, self.status = why, status


_FIXED = None


class Walk:
    """One decode of a whole stream, kept so that the many calls a test makes on pieces of that stream need not decode
    its leading blocks again: a block whose bits all lie inside a call's input decodes to the same bytes whatever
    follows it, in either way of reading, so decode() may start at the last boundary of the walk that the input and the
    budget still reach and decode from there as usual.  body: the bit of the stream (container included) at which
    the deflate blocks start.  tests/test_resume_model.py holds decode() with a walk against decode() without."""

    def __init__(self, data, body=0):
        kept = []
        marks = decode(data, body, b"", 1 << 62, False, keep=kept)[4]
        self.plain, self.bits, self.outs = kept[0], [m[0] for m in marks], [m[1] for m in marks]
        self.at = {b: k for k, b in reversed(list(enumerate(self.bits)))}  # (empty blocks: the first mark at a bit)


def decode(data, bit, window, max_out, last, trace=None, walk=None, origin=0, keep=None):
    """Whole blocks of `data` from bit position `bit` on, `window` being the output before them, until the final
    block, the end of the input or a block that passes max_out.  -> (bytes of the whole blocks, the bit behind them,
    why, status, [(bit, bytes made so far) of every boundary passed, the first included]); status != OK: the stream is
    damaged.  trace: a list that takes (what, bit) of every cut that answered NEED_INPUT.  walk, origin: a Walk of the
    stream that `data` is a piece of, and the stream's bit at which the piece starts.  keep: a list that takes the bytes
    of the whole blocks whatever the status."""
    global _FIXED
    out = bytearray(window)
    base = len(out)
    nbits = len(data) * 8
    pos = bit
    frombytes = int.from_bytes

    def peek(at):
        return frombytes(data[at >> 3:(at >> 3) + 9], "little") >> (at & 7)

    def want(what):  # the bits below pos have been read
        if pos > nbits and not last:
            if trace is not None:
                trace.append((what, pos))
            raise _Stop(NEED_INPUT)

    def bits(n):
        nonlocal pos
        v = peek(pos) & ((1 << n) - 1)
        pos += n
        return v

    def symbol(tab, maxlen, limit, what):
        """the code at pos -> (symbol, its length); None: no code claims the pattern"""
        nonlocal pos
        e = tab[peek(pos) & ((1 << maxlen) - 1)]
        if e:
            pos += e & 15
            want(what)
            return e >> 4
        if pos + limit > nbits and not last:
            if trace is not None:
                trace.append((what, pos))
            raise _Stop(NEED_INPUT)
        return None

    def room():
        if len(out) - base > max_out:
            raise _Stop(NEED_OUTPUT)

    marks = []
    good = (pos, base)
    why, status = DONE, OK
    if walk is not None and origin + pos in walk.at:
        # the furthest boundary whose blocks all lie inside the input and the budget; never the walk's last mark (the
        # closing one of a walk that ended by itself is no block start); the marks then start there
        k0 = walk.at[origin + pos]
        k = min(bisect.bisect_right(walk.bits, origin + nbits), bisect.bisect_right(walk.outs, walk.outs[k0] + max_out),
                len(walk.bits) - 1) - 1
        k = max(k, k0)
        out += walk.plain[walk.outs[k0]:walk.outs[k]]
        pos = walk.bits[k] - origin
    try:
        while True:
            good = (pos, len(out))
            marks.append((pos, len(out) - base))
            final, btype = bits(1), bits(2)
            want("block header")
            if btype == 0:
                pos = (pos + 7) & ~7
                n, nn = bits(16), bits(16)
                want("stored LEN")
                if n + nn != 65535:
                    raise _Stop(None, INVALID_BUFFER)
                if (pos >> 3) + n > len(data):
                    if trace is not None and not last:
                        trace.append(("stored data", pos))
                    raise _Stop(NEED_INPUT) if not last else _Stop(None, END_OF_BUFFER)
                out += data[pos >> 3:(pos >> 3) + n]
                pos += 8 * n
                room()
            elif btype == 3:
                raise _Stop(None, BLOCK_HEADER)
            else:
                if btype == 1:
                    if _FIXED is None:
                        _FIXED = (_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _table([5] * 30))
                    (lit, lit_max), (dist, dist_max) = _FIXED
                else:
                    hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                    want("dynamic counts")
                    if hlit > 286 or hdist > 30:
                        raise _Stop(None, INVALID_BUFFER)
                    cl = [0] * 19
                    for k in range(hclen):
                        cl[CL_ORDER[k]] = bits(3)
                    want("code-length code")
                    cl_tab, cl_max = _table(cl)
                    lens = []
                    total = hlit + hdist
                    while len(lens) != total:
                        sym = symbol(cl_tab, cl_max, 7, "code-length loop")
                        if pos > nbits:
                            raise _Stop(None, END_OF_BUFFER)
                        if sym is None:
                            raise _Stop(None, INVALID_SYMBOL)
                        if sym <= 15:
                            lens.append(sym)
                        elif sym == 16:
                            if not lens:
                                raise _Stop(None, INVALID_BUFFER)
                            rep = 3 + bits(2)
                            want("code-length loop")
                            if len(lens) + rep > 320:
                                raise _Stop(None, INVALID_BUFFER)
                            lens += [lens[-1]] * rep
                        else:
                            rep = 3 + bits(3) if sym == 17 else 11 + bits(7)
                            want("code-length loop")
                            lens += [0] * rep
                        if len(lens) > total:
                            raise _Stop(None, INVALID_BUFFER)
                    (lit, lit_max), (dist, dist_max) = _table(lens[:hlit]), _table(lens[hlit:])
                while True:
                    sym = symbol(lit, lit_max, 15, "literal/length code")
                    if sym is None or sym > 285:
                        raise _Stop(None, INVALID_BUFFER)
                    if sym <= 256:
                        if pos > nbits:
                            raise _Stop(None, END_OF_BUFFER)
                        if sym == 256:
                            break
                        out.append(sym)
                        room()
                        continue
                    k = sym - 257
                    length = LEN_BASE[k] + bits(LEN_EXTRA[k])
                    want("length extra bits")
                    d = symbol(dist, dist_max, 15, "distance code")
                    if d is None or d >= 30:
                        raise _Stop(None, INVALID_BUFFER)
                    distance = DIST_BASE[d] + bits(DIST_EXTRA[d])
                    want("distance extra bits")
                    if pos > nbits:
                        raise _Stop(None, END_OF_BUFFER)
                    if distance > len(out):
                        raise _Stop(None, INVALID_BUFFER)
                    at = len(out) - distance
                    if distance >= length:
                        out += out[at:at + length]
                    else:
                        for i in range(length):
                            out.append(out[at + i])
                    room()
            if final:
                good = (pos, len(out))
                marks.append((pos, len(out) - base))
                break
    except _Stop as s:
        why, status = s.why, s.status
    except Fail:  # an over-subscribed code
        why, status = None, INVALID_BUFFER
    if keep is not None:
        keep.append(bytes(out[base:good[1]]))
    if status != OK:
        return b"", bit, None, status, marks
    return bytes(out[base:good[1]]), good[0], why, OK, marks


# ---- one call of one stream ----
def step(state, data, max_out, last=False, fmt=DF_DETECT, trace=None, walk=None):
    """-> (out, consumed, state', why, status); a stream that fails has no output, no state and nothing consumed.
    walk: a Walk of the stream that this call's input is a piece of (the state, if any, being a true one)."""
    assert max_out > 0
    data = bytes(data)
    bad = lambda status: (b"", 0, None, None, status)
    if state is None:
        status, need, fmt, body = read_head(data, fmt, last)
        if status != OK:
            return bad(status)
        if need:
            if trace is not None:
                trace.append(("container header", 8 * len(data)))
            return b"", 0, None, NEED_INPUT, OK
        s = State(pack_state(fmt, 1, 0, 0, 0, 1 if fmt == DF_ZLIB else 0, b""))
    else:
        if not sound(state):
            return bad(INVALID_BUFFER)
        s, body = State(state), 0
    tl = trailer_bytes(s.fmt)
    if s.phase == 2:
        if len(data) < tl:
            if trace is not None and not last:
                trace.append(("trailer", 8 * len(data)))
            return bad(CHECKSUM) if last else (b"", 0, bytes(state), NEED_INPUT, OK)
        status = check_trailer(data, s.fmt, s.check, s.total_out)
        return bad(status) if status != OK else (b"", tl, None, DONE, OK)
    out, bit, why, status, _ = decode(data, 8 * body + s.bit_skip, s.window, max_out, last, trace, walk, 8 * s.total_in)
    if status != OK:
        return bad(status)
    s.total_out += len(out)
    if s.fmt == DF_GZIP:
        s.check = crc32(out, s.check)
    elif s.fmt == DF_ZLIB:
        s.check = adler32(out, s.check)
    used, s.bit_skip = bit >> 3, bit & 7
    if why == DONE:
        used, s.bit_skip = (bit + 7) >> 3, 0
        if used + tl > len(data):
            if last:
                return bad(CHECKSUM)
            if trace is not None:
                trace.append(("trailer", 8 * len(data)))
            s.phase, why = 2, NEED_INPUT
        else:
            status = check_trailer(data[used:], s.fmt, s.check, s.total_out)
            if status != OK:
                return bad(status)
            return out, used + tl, None, DONE, OK
    s.total_in += used
    s.window = (s.window + out)[-min(s.total_out, WINDOW):] if s.total_out else b""
    s.win_len = len(s.window)
    return out, used, s.pack(), why, OK
