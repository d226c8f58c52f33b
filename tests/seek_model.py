"""A model of the seek index (include/zippy_hip.h: zh_seek_index_batch, zh_seek_read_ranges) in plain Python, written
from RFC 1951 and the header's prose: an inflate that starts at any bit position with a given window, stops at a given
bit and reports every block start; the point rule; the blob writer and reader; the arithmetic of a range read (the
intervals a range touches, the bytes its upload carries).  No engine and no zlib in here: tests/test_seek_model.py
holds it against zlib.decompress."""
import functools
import struct
import zlib

from deflate_craft import CL_ORDER, DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA

WINDOW = 32768
DEFAULT_SPAN = 1 << 20
MAGIC = b"ZHSKIDX1"
DF_DETECT, DF_ZLIB, DF_GZIP, DF_DEFLATE = 0, 1, 2, 3
OK, INVALID_BUFFER, CHECKSUM = 0, 13, 8


class Fail(Exception):
    """the stream cannot be decoded (what the engine answers with a decoder status or ZH_ERR_INVALID_BUFFER)"""


def _table(lens):
    """(lookup table over maxlen reversed bits -> sym << 4 | len, maxlen); 0: no code.  Over-subscribed sets fail,
    incomplete ones are taken (their unclaimed patterns fail when met)."""
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for bits in range(1, 16):
        nxt[bits] = code
        code += count[bits]
        if code > (1 << bits):
            raise Fail("over-subscribed")
        code <<= 1
    maxlen = max([n for n in lens if n] or [1])
    tab = [0] * (1 << maxlen)
    for sym, n in enumerate(lens):
        if n:
            c = nxt[n]
            nxt[n] += 1
            rev = int(format(c, "0%db" % n)[::-1], 2)
            tab[rev::1 << n] = [sym << 4 | n] * (1 << (maxlen - n))
    return tab, maxlen


_FIXED = None


def inflate(data, bit=0, window=b"", stop=None, limit=None):
    """Decodes deflate blocks of `data` from bit position `bit`, `window` being the output before them.  Ends behind a
    final block, or, with `stop`, at the block boundary at that bit (a boundary beyond it, or a final block that ends
    elsewhere, fails).  limit: the most bytes it may make.  -> (bytes made, [(bit_off, out_off) of every block start,
    out_off counted from the first byte made], the bit it ended at)"""
    global _FIXED
    out = bytearray(window)
    base = len(out)
    end_bits = len(data) * 8
    pos = bit
    blocks = []
    frombytes = int.from_bytes

    def bits(n):
        nonlocal pos
        v = (frombytes(data[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << n) - 1)
        pos += n
        return v

    while True:
        if stop is not None and pos >= stop:
            if pos > stop:
                raise Fail("a block boundary beyond the stop bit")
            break
        blocks.append((pos, len(out) - base))
        final, btype = bits(1), bits(2)
        if pos > end_bits:
            raise Fail("end of buffer")
        if btype == 0:
            pos = (pos + 7) & ~7
            n, nn = bits(16), bits(16)
            if pos > end_bits or n + nn != 65535 or (pos >> 3) + n > len(data):
                raise Fail("stored block")
            out += data[pos >> 3:(pos >> 3) + n]
            pos += 8 * n
        elif btype == 3:
            raise Fail("block type 3")
        else:
            if btype == 1:
                if _FIXED is None:
                    _FIXED = (_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _table([5] * 30))
                (lit, lit_max), (dist, dist_max) = _FIXED
            else:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                if hlit > 286 or hdist > 30:
                    raise Fail("HLIT / HDIST")
                cl = [0] * 19
                for k in range(hclen):
                    cl[CL_ORDER[k]] = bits(3)
                cl_tab, cl_max = _table(cl)
                lens = []
                while len(lens) < hlit + hdist:
                    e = cl_tab[(frombytes(data[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << cl_max) - 1)]
                    if not e:
                        raise Fail("no code-length code")
                    pos += e & 15
                    sym = e >> 4
                    if pos > end_bits:
                        raise Fail("end of buffer")
                    if sym <= 15:
                        lens.append(sym)
                    elif sym == 16:
                        if not lens:
                            raise Fail("repeat of nothing")
                        lens += [lens[-1]] * (3 + bits(2))
                    elif sym == 17:
                        lens += [0] * (3 + bits(3))
                    else:
                        lens += [0] * (11 + bits(7))
                if len(lens) > hlit + hdist:
                    raise Fail("too many code lengths")
                (lit, lit_max), (dist, dist_max) = _table(lens[:hlit]), _table(lens[hlit:])
            lit_mask, dist_mask = (1 << lit_max) - 1, (1 << dist_max) - 1
            while True:
                v = frombytes(data[pos >> 3:(pos >> 3) + 8], "little") >> (pos & 7)
                e = lit[v & lit_mask]
                if not e:
                    raise Fail("no literal/length code")
                n = e & 15
                sym = e >> 4
                if sym < 256:
                    pos += n
                    if pos > end_bits:
                        raise Fail("end of buffer")
                    out.append(sym)
                    continue
                if sym == 256:
                    pos += n
                    if pos > end_bits:
                        raise Fail("end of buffer")
                    break
                if sym > 285:
                    raise Fail("length symbol")
                v >>= n
                k = sym - 257
                length = LEN_BASE[k] + (v & ((1 << LEN_EXTRA[k]) - 1))
                v >>= LEN_EXTRA[k]
                n += LEN_EXTRA[k]
                e = dist[v & dist_mask]
                if not e:
                    raise Fail("no distance code")
                v >>= e & 15
                n += e & 15
                d = e >> 4
                if d >= 30:
                    raise Fail("distance symbol")
                distance = DIST_BASE[d] + (v & ((1 << DIST_EXTRA[d]) - 1))
                pos += n + DIST_EXTRA[d]
                if pos > end_bits:
                    raise Fail("end of buffer")
                if distance > len(out):
                    raise Fail("distance beyond the window")
                at = len(out) - distance
                if distance >= length:
                    out += out[at:at + length]
                else:
                    for i in range(length):
                        out.append(out[at + i])
                if limit is not None and len(out) - base > limit:
                    raise Fail("more bytes than promised")
        if limit is not None and len(out) - base > limit:
            raise Fail("more bytes than promised")
        if final:
            if stop is not None and pos != stop:
                raise Fail("the final block ends elsewhere")
            break
    return bytes(out[base:]), blocks, pos


def resolve_format(data, fmt):
    if fmt != DF_DETECT:
        return fmt
    if len(data) > 18 and data[0] == 31 and data[1] == 139 and data[2] == 8 and not data[3] & 0xe0:
        return DF_GZIP
    assert len(data) > 6 and data[0] & 15 == 8 and data[0] >> 4 <= 7 and (data[0] * 256 + data[1]) % 31 == 0
    return DF_ZLIB


def body_bit(data, fmt):
    """the first bit of the deflate body (the tests' gzip headers carry at most a name and a comment)"""
    if fmt == DF_GZIP:
        p = 10
        for flag in (8, 16):
            if data[3] & flag:
                p = data.index(0, p) + 1
        return 8 * (p + (2 if data[3] & 2 else 0))
    return 16 if fmt == DF_ZLIB else 0


def choose_points(blocks, end_bit, total, span):
    """the point rule: [(bit_off, out_off)], the closing entry last"""
    points = [blocks[0]]
    for b in blocks[1:]:
        if b[1] - points[-1][1] >= span:
            points.append(b)
    return points + [(end_bit, total)]


def pad16(n):
    return (n + 15) & ~15


def write_blob(fmt, src_len, span, points, plain):
    """the blob of a stream whose chosen points (closing entry included) and plaintext are known"""
    recs, store = [], bytearray()
    for k, (bit_off, out_off) in enumerate(points):
        closing = k + 1 == len(points)
        win = b"" if closing else plain[max(0, out_off - WINDOW):out_off]
        crc = 0 if closing else zlib.crc32(plain[out_off:points[k + 1][1]])
        recs.append(struct.pack("<QQQII", bit_off, out_off, len(store), len(win), crc))
        store += win + bytes(pad16(len(win)) - len(win))
    head = MAGIC + struct.pack("<IIQQQQQQ", 1, fmt, src_len, len(plain), span, len(points), len(store), 0)
    assert len(head) == 64
    return head + b"".join(recs) + bytes(store)


def build_index(data, fmt=DF_DETECT, span=0):
    """-> (blob, plaintext) of a sound stream"""
    span = span or DEFAULT_SPAN
    assert span >= WINDOW
    fmt = resolve_format(data, fmt)
    plain, blocks, end_bit = inflate(data, body_bit(data, fmt))
    return write_blob(fmt, len(data), span, choose_points(blocks, end_bit, len(plain), span), plain), plain


class Blob:
    """a blob taken apart (no checks: the tests damage blobs through this as well)"""

    def __init__(self, blob):
        (self.magic, self.version, self.fmt, self.src_len, self.total, self.span, self.n_points, self.window_bytes,
         self.reserved) = struct.unpack_from("<8sIIQQQQQQ", blob, 0)
        self.points = [list(struct.unpack_from("<QQQII", blob, 64 + 32 * k)) for k in range(self.n_points)]
        self.store = bytes(blob[64 + 32 * self.n_points:])

    def pack(self):
        head = struct.pack("<8sIIQQQQQQ", self.magic, self.version, self.fmt, self.src_len, self.total, self.span,
                           self.n_points, self.window_bytes, self.reserved)
        return head + b"".join(struct.pack("<QQQII", *p) for p in self.points) + self.store

    def window(self, k):
        p = self.points[k]
        return self.store[p[2]:p[2] + p[3]]

    def interval_of(self, byte):
        """the interval k with out_off[k] <= byte < out_off[k + 1]"""
        k = 0
        while self.points[k + 1][1] <= byte:
            k += 1
        return k

    def touched(self, off, length):
        """the intervals k0 .. k1 a range touches after clipping ([] for a range of no bytes)"""
        end = min(self.total, off + length)
        if off >= self.total or end <= off:
            return []
        return list(range(self.interval_of(off), self.interval_of(end - 1) + 1))


def decode_interval(data, blob, k):
    """What the engine makes of interval k: (OK, bytes), (CHECKSUM, None) where the interval decodes to its promised
    length and stops where it should but its bytes are not the indexed ones, (INVALID_BUFFER, None) where it does not
    (the engine: a decoder status or ZH_ERR_INVALID_BUFFER)."""
    p, q = blob.points[k], blob.points[k + 1]
    try:
        got, _, _ = inflate(data, p[0], blob.window(k), stop=q[0], limit=q[1] - p[1])
    except Fail:
        return INVALID_BUFFER, None
    if len(got) != q[1] - p[1]:
        return INVALID_BUFFER, None
    return (OK, got) if zlib.crc32(got) == p[4] else (CHECKSUM, None)


def upload_bytes(blobs, src_lens, ranges):
    """The bytes a zh_seek_read_ranges call sends over the link: per live range the compressed span [bit_off[k0] / 8,
    ceil(bit_off[k1 + 1] / 8)) of its stream and the padded windows of its non-empty intervals; spans of one owner (a
    stream's bytes, a stream's window store) that overlap or touch are one; every merged span starts at the next
    multiple of 16."""
    spans = []
    for s, off, length in ranges:
        b = blobs[s]
        ks = b.touched(off, length)
        if not ks:
            continue
        spans.append((2 * s, b.points[ks[0]][0] // 8, min((b.points[ks[-1] + 1][0] + 7) // 8, src_lens[s])))
        for k in ks:
            if b.points[k][3] and b.points[k + 1][1] > b.points[k][1]:
                spans.append((2 * s + 1, b.points[k][2], b.points[k][2] + pad16(b.points[k][3])))
    spans.sort()
    merged = []
    for owner, lo, hi in spans:
        if merged and merged[-1][0] == owner and lo <= merged[-1][2]:
            merged[-1][2] = max(merged[-1][2], hi)
        else:
            merged.append([owner, lo, hi])
    total = 0
    for _, lo, hi in merged:
        total = pad16(total) + hi - lo
    return total


@functools.lru_cache(maxsize=64)
def walk(data, fmt):
    """inflate() of a whole stream of a resolved format, made once a stream: (plaintext, block starts, end bit)"""
    return inflate(data, body_bit(data, fmt))


def index_at(data, fmt, keep, span=WINDOW):
    """The blob whose points are the first block and the true block starts j = 1, 2 .. for which keep(j, (bit_off,
    out_off)) holds, and the closing entry -- whatever the point rule would choose.  -> (blob, plaintext)"""
    fmt = resolve_format(data, fmt)
    plain, blocks, end_bit = walk(data, fmt)
    points = [b for j, b in enumerate(blocks) if j == 0 or keep(j, b)]
    return write_blob(fmt, len(data), span, points + [(end_bit, len(plain))], plain), plain


def sound(blob, src_len):
    """The rules of include/zippy_hip.h for a blob that can be right, one by one in the order of its prose: what a
    reader may say of a blob without decoding anything."""
    if len(blob) < 64:
        return False
    magic, version, _, _, _, _, n_points, window_bytes, _ = struct.unpack_from("<8sIIQQQQQQ", blob, 0)
    if magic != MAGIC or version != 1:
        return False
    if len(blob) != 64 + 32 * n_points + window_bytes:          # a length that does not match its own counts
        return False
    b = Blob(blob)
    if b.src_len != src_len or b.n_points < 2:
        return False
    p = b.points
    if p[0][1] != 0 or p[-1][1] != b.total:                     # (the closing entry holds `total`)
        return False
    for k, (bit_off, out_off, win_off, win_len, _) in enumerate(p):
        closing = k + 1 == len(p)
        if bit_off > 8 * src_len if closing else bit_off >= 8 * src_len:
            return False
        if win_len != (0 if closing else min(out_off, WINDOW)):
            return False
        if win_off % 16 or win_off + pad16(win_len) > b.window_bytes:
            return False
        if closing:
            break
        if p[k + 1][0] <= bit_off or p[k + 1][1] < out_off:     # bit_off strictly rising, out_off not falling
            return False
        if p[k + 1][1] - out_off > 1032 * ((p[k + 1][0] + 7) // 8 - bit_off // 8) + 64:
            return False
    return True


def decoded(blob, off, length):
    """the intervals of a range the engine decodes: those it touches that are not empty"""
    return [k for k in blob.touched(off, length) if blob.points[k + 1][1] > blob.points[k][1]]
