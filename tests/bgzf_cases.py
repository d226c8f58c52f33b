"""Shared by tests/test_emu_bgzf.py and tests/test_gpu_bgzf.py: BGZF files made member by member, and the checks of
zh_bgzf_write_batch / zh_bgzf_read_batch / zh_bgzf_index_batch / zh_bgzf_read_ranges (Engine.bgzf_*) against
tests/bgzf_model.py.  Where the model's decoder (the oracle) rejects a stream, the status to equal is the one
Engine.uncompress_batch gives the same bytes, as in tests/zip_read_cases.py.

The scan's geometry (zh_scan.h): a lane reads 16 bytes, a wave 1024, a workgroup 16384; the walk's scan covers 1024
nodes a workgroup; the assemble kernel moves 4096 bytes of CDATA a wave."""
import gzip
import random
import struct
import zlib

import pytest

import bgzf_model as bm
import deflate_craft as dc
import oracle
from zippy_amd.common import ZippyError

LEVELS = (-2, 0, 1, 6, 9)
BLOCKS = (7, 4096, 65280, 65505)


def lengths(b):
    return (0, 1, b - 1, b, b + 1, 2 * b, 3 * b + 17)


def pattern(n, seed=1):
    """text-like bytes with long and short repeats, some noise in between"""
    rng = random.Random(seed * 7919 + n)
    out = bytearray()
    words = [bytes(rng.randrange(97, 123) for _ in range(rng.randrange(2, 9))) for _ in range(40)]
    while len(out) < n:
        k = rng.randrange(10)
        if k == 0:
            out += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 60)))
        elif k == 1:
            out += bytes([rng.randrange(256)]) * rng.randrange(1, 300)
        else:
            out += rng.choice(words) + b" "
    return bytes(out[:n])


def noise(n, seed=3):
    return random.Random(seed).randbytes(n)


def decoder(eng):
    """the oracle's inflate; where it fails, the codec's own status for the same bytes"""
    cache = {}

    def decode(cdata):
        if cdata not in cache:
            st, out = bm.oracle_decoder(cdata)
            if st != bm.OK:
                st = eng.uncompress_batch([cdata], 3)[1][0]
                assert st != bm.OK
            cache[cdata] = (st, out)
        return cache[cdata]
    return decode


# ---------------------------------------------------------------------------
# writing
# ---------------------------------------------------------------------------
_written = {}


def written(src, level, b):
    """the model's file, made once"""
    key = (src, level, b)
    if key not in _written:
        _written[key] = bm.write(src, level, b)
    return _written[key]


def check_write(eng, srcs, level, b):
    """one call: byte-identical to the model, and any gunzip recovers the source"""
    outs, sts = eng.bgzf_compress_batch(srcs, level, b)
    assert sts == [0] * len(srcs)
    for src, out in zip(srcs, outs):
        assert out == written(src, level, b), (len(src), level, b)
        assert gzip.decompress(out) == src
    return outs


def check_write_matrix(eng, levels=LEVELS, blocks=BLOCKS):
    for b in blocks:
        srcs = [pattern(n, 1 + i) for i, n in enumerate(lengths(b))]
        for level in levels:
            outs = check_write(eng, srcs, level, b)
            check_read(eng, outs, want=[bm.OK] * len(srcs), datas=srcs)  # (read and index: everything written)


def check_write_33(eng):
    sizes = [0, 1, 4095, 4096, 4097, 0, 12000, 3, 0, 8192, 100] * 3
    assert len(sizes) == 33
    srcs = [pattern(n, 50 + i) if i % 4 else noise(n, i) for i, n in enumerate(sizes)]
    outs = check_write(eng, srcs, 1, 4096)
    check_read(eng, outs, want=[bm.OK] * 33)


def check_write_residues(eng):
    """b = 7 over 1000 bytes: member starts at every residue mod 16"""
    src = pattern(1000, 9)
    out = check_write(eng, [src], 6, 7)[0]
    st, idx, eof = bm.index(out)
    assert {c % 16 for c, _ in idx} == set(range(16))
    check_read(eng, [out], want=[bm.OK])


def check_write_whole_chunks(eng):
    """1700 bytes of noise at level 0, b = 100: every member is 18 + 105 + 8 = 131 bytes, and 131 mod 16 = 3 is coprime
    to 16 -- the CDATA of sixteen consecutive members starts at every residue mod 16, each with five or six whole 16-byte
    chunks (check_write_residues' members are shorter than 30 bytes: no whole chunk)"""
    src = noise(1700, 5)
    out = check_write(eng, [src], 0, 100)[0]
    st, idx, eof = bm.index(out)
    assert [c for c, _ in idx[:17]] == [131 * k for k in range(17)]
    assert {(c + 18) % 16 for c, _ in idx[:16]} == set(range(16))
    assert all((c + 18 + 105) // 16 - (c + 18 + 15) // 16 >= 5 for c, _ in idx[:16])
    check_read(eng, [out], want=[bm.OK])


def fallback_pair():
    return noise(65505, 11), noise(65450, 12)


def check_fallback(eng):
    """random bytes at level -2 outgrow a member at 65 505 bytes and do not at 65 450 (the oracle says so)"""
    big, small = fallback_pair()
    assert len(oracle.compress(big, -2, oracle.dfDeflate)) > bm.MAX_CDATA
    assert len(oracle.compress(small, -2, oracle.dfDeflate)) <= bm.MAX_CDATA
    outs = check_write(eng, [big, small, big + small], -2, 65505)
    assert len(outs[0]) == 18 + 5 + 65505 + 8 + 28
    check_read(eng, outs, want=[bm.OK] * 3)


def check_contract_mode(eng):
    """the parallel BestSpeed parse writes other bytes: the round trip only"""
    srcs = [pattern(n, 70 + i) for i, n in enumerate((0, 5, 70000, 200000))]
    eng.set_l1_parse(1)
    try:
        outs, sts = eng.bgzf_compress_batch(srcs, 1, 0)
    finally:
        eng.set_l1_parse(-1)
    assert sts == [0] * 4
    assert [gzip.decompress(o) for o in outs] == srcs
    back, sts = eng.bgzf_uncompress_batch(outs)
    assert (back, sts) == (srcs, [0] * 4)


def check_write_errors(eng):
    for level in (-3, 10):
        with pytest.raises(ZippyError) as e:
            eng.bgzf_compress_batch([b"abc"], level, 0)
        assert e.value.status == bm.INVALID_LEVEL
    for b in (65506, 1 << 20):
        with pytest.raises(ZippyError) as e:
            eng.bgzf_compress_batch([b"abc"], 1, b)
        assert e.value.status == bm.ARGUMENT
    assert eng.bgzf_compress_batch([], 1, 0) == ([], [])
    assert eng.bgzf_compress_batch([b"xyz"], 1, 65505)[0] == [written(b"xyz", 1, 65505)]


# ---------------------------------------------------------------------------
# images
# ---------------------------------------------------------------------------
def raw(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def mem(data, cdata=None, extra=None, crc=None, isize=None, bsize=None, head=b"\x1f\x8b\x08\x04", xlen=None):
    """a member; extra: the subfields in front of BC"""
    cdata = raw(data) if cdata is None else cdata
    extra = b"" if extra is None else extra
    total = 12 + len(extra) + 6 + len(cdata) + 8
    fields = extra + b"BC\x02\x00" + struct.pack("<H", (total - 1 if bsize is None else bsize) & 0xFFFF)
    return (head + b"\0\0\0\0\0\xff" + struct.pack("<H", len(fields) if xlen is None else xlen) + fields + cdata +
            struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) if isize is None else isize))


def subfield(tag, data):
    return tag + struct.pack("<H", len(data)) + data


def flushed_member(data):
    """one member of several deflate blocks: zlib with a full flush inside"""
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    half = len(data) // 2
    cdata = c.compress(data[:half]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[half:]) + c.flush()
    return mem(data, cdata)


def crafted_member():
    """a stored block with odd padding, then a fixed block with a match, by hand"""
    s = dc.Stream()
    s.stored(b"stored bytes ", False, pad_bits=0x15)
    s.fixed_block(True)
    for ch in b"abcabc":
        s.lit(ch)
    s.match(9, 3)
    s.eob()
    cdata, plain, st = s.finish()
    assert st is None
    return mem(bytes(plain), cdata), bytes(plain)


def stored_cdata(data):
    return b"\x01" + struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data


def good_images():
    """-> [(name, image, data)]"""
    a, b, c = pattern(5000, 21), pattern(300, 22), noise(900, 23)
    crafted, crafted_plain = crafted_member()
    fake = mem(b"never a member") + bm.EOF  # a whole file inside a stored block
    out = [
        ("empty", b"", b""),
        ("marker alone", bm.EOF, b""),
        ("zlib members", mem(a) + mem(b) + bm.EOF, a + b),
        ("several deflate blocks", flushed_member(a) + flushed_member(c) + bm.EOF, a + c),
        ("crafted", crafted + bm.EOF, crafted_plain),
        ("subfield before BC", mem(a, extra=subfield(b"XY", b"12345")) + mem(b, extra=subfield(b"BC", b"123")) + bm.EOF, a + b),
        ("two files", mem(a) + bm.EOF + mem(b) + mem(c) + bm.EOF, a + b + c),
        ("no marker", mem(a) + mem(b), a + b),
        ("signature in stored data", mem(b) + mem(fake, stored_cdata(fake)) + mem(fake + b"\x1f\x8b\x08", stored_cdata(fake + b"\x1f\x8b\x08")) + bm.EOF,
         b + fake + fake + b"\x1f\x8b\x08"),
    ]
    for k in (13, 14, 15):  # the second member starts at offset k of a 16-byte chunk
        first = mem(b, extra=subfield(b"PD", b""))
        first = mem(b, extra=subfield(b"PD", b"\0" * ((k - len(first)) % 16)))
        assert len(first) % 16 == k
        out.append(("start at %d" % k, first + mem(a) + bm.EOF, b + a))
    return out


def many_members():
    """1600 members (b = 64): past the scan's 1024-item group, 11 doubling rounds"""
    src = pattern(1600 * 64, 31)
    return written(src, 1, 64), src


def bad_images():
    """-> [(name, image, status the case is built for | None: the decoder's)]"""
    a, b = pattern(3000, 41), pattern(200, 42)
    good = mem(a) + mem(b)
    m = mem(a)
    cd = raw(a)
    damaged = bytearray(cd)
    damaged[len(cd) // 2] ^= 0x55
    damaged[len(cd) // 2 + 1] ^= 0xAA
    five = [mem(pattern(100 + i, 60 + i)) for i in range(6)]
    return [
        ("5 bytes left", good + b"\x1f\x8b\x08\x04\x00", bm.INVALID_BUFFER),
        ("junk behind", good + bm.EOF + b"\0" * 40, bm.GZIP_ID),
        ("id at byte 0", b"\x1f\x8c" + m[2:], bm.GZIP_ID),
        ("method", good + mem(b, head=b"\x1f\x8b\x07\x04"), bm.UNSUPPORTED_METHOD),
        ("reserved flag", good + mem(b, head=b"\x1f\x8b\x08\x24"), bm.RESERVED_FLAGS),
        ("plain gzip", gzip.compress(b), bm.UNSUPPORTED_FLAGS),
        ("fname flag too", mem(b, head=b"\x1f\x8b\x08\x0c"), bm.UNSUPPORTED_FLAGS),
        ("xlen past the image", m[:10] + struct.pack("<H", 5000) + m[12:200], bm.INVALID_BUFFER),
        ("no BC", mem(b)[:12] + b"BD" + mem(b)[14:], bm.BGZF_HEADER),
        ("BC of three bytes", b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x07\x00BC\x03\x00\x30\x00\x00" + b"\0" * 40, bm.BGZF_HEADER),
        ("subfields do not tile", mem(b, xlen=7) + b"\0" * 8, bm.BGZF_HEADER),
        ("subfield past xlen", mem(b, extra=b"XY\x40\x00"), bm.BGZF_HEADER),
        ("bsize too small", good + mem(b, bsize=20), bm.BGZF_HEADER),
        ("isize too large", good + mem(b, isize=65537), bm.BGZF_HEADER),
        ("cut in the header", good + m[:9], bm.INVALID_BUFFER),
        ("cut in the extra field", good + m[:15], bm.INVALID_BUFFER),
        ("cut in cdata", good + m[:len(m) // 2], bm.INVALID_BUFFER),
        ("cut in the trailer", good + m[:-3], bm.INVALID_BUFFER),
        ("isize one more", mem(b) + mem(a, isize=len(a) + 1) + bm.EOF, bm.SIZE),
        ("isize one less", mem(b) + mem(a, isize=len(a) - 1) + bm.EOF, bm.SIZE),
        ("crc flipped", mem(b) + mem(a, crc=zlib.crc32(a) ^ 1) + bm.EOF, bm.CHECKSUM),
        ("deflate byte damaged", mem(b) + mem(a, bytes(damaged)) + bm.EOF, None),
        ("crc in 2, header in 5", five[0] + five[1] + mem(b, crc=5) + five[3] + five[4] + mem(b, head=b"\x1f\x8b\x09\x04") + bm.EOF,
         bm.CHECKSUM),
        ("header in 2, crc in 5", five[0] + five[1] + mem(b, bsize=3) + five[3] + five[4] + mem(b, crc=5) + bm.EOF, bm.BGZF_HEADER),
    ]


def straddling_pair():
    """a signature that begins in an image's last three bytes, the next image supplying the rest: neither becomes a
    member (the images lie next to each other in the upload when the first one's length is a multiple of 8)"""
    b = pattern(200, 43)
    first = mem(b) + bm.EOF + b"\x1f\x8b\x08"
    first = mem(b, extra=subfield(b"PD", b"\0" * ((4 - len(first)) % 8))) + bm.EOF + b"\x1f\x8b\x08"
    assert len(first) % 8 == 0
    second = b"\x04" + mem(b)[4:] + bm.EOF
    return [first, second], [bm.INVALID_BUFFER, bm.GZIP_ID]


# ---------------------------------------------------------------------------
# reading and indexing
# ---------------------------------------------------------------------------
def check_read(eng, images, want=None, datas=None):
    """`images` in ONE call of read and of index, held against the model (and against `want`, the statuses the cases
    were built for; None: the decoder's).  -> what the read returned"""
    images = [bytes(x) for x in images]
    dec = decoder(eng)
    outs, sts, eofs = eng.bgzf_uncompress_batch(images, want_eof=True)
    idxs, ists, ieofs = eng.bgzf_index_batch(images)
    assert len(outs) == len(sts) == len(eofs) == len(idxs) == len(ists) == len(images)
    for t, image in enumerate(images):
        tag = "image %d" % t
        st, data, eof = bm.read(image, dec)
        if want is not None and want[t] is not None:
            assert st == want[t], "%s: the model says %r, built for %r" % (tag, st, want[t])
        if want is not None and want[t] is None:
            assert st != bm.OK, tag
        assert sts[t] == st, "%s: status %d, the model says %d" % (tag, sts[t], st)
        assert outs[t] == data, tag
        assert eofs[t] == eof, tag
        if datas is not None and st == bm.OK:
            assert data == datas[t], tag
        ist, idx, ieof = bm.index(image)
        assert (ists[t], idxs[t], ieofs[t]) == (ist, idx, ieof), tag
    return outs, sts


def check_good_images(eng):
    cases = good_images()
    check_read(eng, [c[1] for c in cases], want=[bm.OK] * len(cases), datas=[c[2] for c in cases])
    for name, image, data in cases:
        assert gzip.decompress(image) == data, name


def check_many_members(eng):
    image, src = many_members()
    outs, sts = check_read(eng, [bm.EOF, image, image[:-28]], want=[bm.OK] * 3, datas=[b"", src, src])


def check_bad_images(eng):
    """every failing case in one call among good ones, and each alone: equal results"""
    cases = bad_images()
    goods = good_images()
    images, want = [], []
    for i, (name, image, st) in enumerate(cases):
        images += [image, goods[i % len(goods)][1]]
        want += [st, bm.OK]
    outs, sts = check_read(eng, images, want=want)
    for t in range(0, len(images), 2):
        one = eng.bgzf_uncompress_batch([images[t]])
        assert (one[0][0], one[1][0]) == (outs[t], sts[t]), cases[t // 2][0]


def check_straddling_pair(eng):
    images, want = straddling_pair()
    check_read(eng, images, want=want)
    check_read(eng, images + [good_images()[2][1]], want=want + [bm.OK])


# ---------------------------------------------------------------------------
# ranges
# ---------------------------------------------------------------------------
RB = 4096  # the members of the range cases


def range_files(n=8, size=9 * RB + 123):
    srcs = [pattern(size + 1000 * i, 80 + i) for i in range(n)]
    return srcs, [written(s, 1, RB) for s in srcs]


def spans_union(indexes, ranges):
    """bytes in the union of the spans [coff[k0], coff[k1 + 1]) of the ranges"""
    spans = []
    for t, off, n in ranges:
        _, _, ks = bm.touched(indexes[t], off, n)
        if ks:
            spans.append((t, indexes[t][ks[0]][0], indexes[t][ks[-1] + 1][0]))
    spans.sort()
    total, cur = 0, None
    for t, lo, hi in spans:
        if cur and cur[0] == t and lo <= cur[2]:
            cur = (t, cur[1], max(cur[2], hi))
        else:
            total += cur[2] - cur[1] if cur else 0
            cur = (t, lo, hi)
    return total + (cur[2] - cur[1] if cur else 0)


def check_ranges(eng, srcs, images, indexes, ranges, want=None):
    """one call against the model, against slices of the sources where a range succeeds, and the upload's size
    between the union of the spans and that plus 15 bytes a range"""
    outs, sts = eng.bgzf_read_ranges(images, indexes, ranges)
    mouts, msts = bm.ranges(images, indexes, ranges, decoder(eng))
    assert sts == msts, (sts, msts)
    assert outs == mouts
    if want is not None:
        assert sts == want
    for (t, off, n), out, st in zip(ranges, outs, sts):
        if st == bm.OK and srcs is not None:
            assert out == srcs[t][off:off + n], (t, off, n)
    up = eng.debug_range_stats()[0]
    sound = [r for r in ranges if bm.index_sound(indexes[r[0]], len(images[r[0]]))]
    U = spans_union(indexes, sound)
    assert U <= up <= U + 15 * max(1, len(ranges)), (U, up)
    return outs, sts


def check_range_shapes(eng):
    srcs, images = range_files(2)
    indexes = [bm.index(x)[1] for x in images]
    total = len(srcs[0])
    ranges = [(0, 100, 50), (0, RB - 10, 20), (0, 0, 1), (0, total - 1, 1), (0, total - 1, 100), (0, total, 5),
              (0, total + 1000, 5), (0, 17, 0), (0, 0, total), (1, 0, 1 << 63), (0, 5, (1 << 64) - 1), (0, RB, RB)]
    check_ranges(eng, srcs, images, indexes, ranges, want=[0] * len(ranges))
    check_ranges(eng, srcs, images, indexes, [(0, RB - 10, 4 * RB)])
    assert eng.debug_range_stats()[1:] == (3, 2)  # across five members: the middle ones in place
    check_ranges(eng, srcs, images, indexes, [(0, RB, 2 * RB)])
    assert eng.debug_range_stats()[1:] == (2, 0)
    check_ranges(eng, srcs, images, indexes, [(0, 10, 20), (0, 15, 30)])  # the same member twice: sent once, decoded twice
    assert eng.debug_range_stats()[1:] == (0, 2)
    # the upload's accounting (check_ranges' bound) where spans merge: neighbours that touch exactly, and the same
    # offsets asked of two images in alternating order
    check_ranges(eng, srcs, images, indexes, [(0, 0, RB), (0, RB, RB)], want=[0, 0])
    check_ranges(eng, srcs, images, indexes, [(1, 100, 50), (0, 100, 50), (1, RB, 10), (0, RB, 10)], want=[0] * 4)
    assert eng.bgzf_read_ranges(images, indexes, []) == ([], [])


def check_range_big_members(eng):
    """members of 65280 bytes: an edge member's clip is cut into pieces of 16 KiB that end on multiples of 16"""
    src = pattern(3 * 65280 + 5, 90)
    image = written(src, 1, 0)
    idx = bm.index(image)[1]
    ranges = [(0, 100, 60000), (0, 3, 65277), (0, 65000, 70000), (0, 16385, 2 * 65280), (0, 65279, 65282 + 16384),
              (0, 1, 16384), (0, 65280 - 16383, 16400), (0, 0, len(src))]
    check_ranges(eng, [src], [image], [idx], ranges, want=[0] * len(ranges))
    assert eng.debug_range_stats()[1:] == (3 + 4, 11)  # whole members in place: one each of three ranges, four of the last


def check_range_residues(eng):
    """all 16 x 16 residues of where a clip starts in its member and of its length"""
    srcs, images = range_files(1, 3 * RB)
    indexes = [bm.index(x)[1] for x in images]
    ranges = [(0, RB + 100 + a, 2 * RB - 300 + b) for a in range(16) for b in range(16)]
    ranges += [(0, 200 + a, 33 + b) for a in range(16) for b in range(16)]
    check_ranges(eng, srcs, images, indexes, ranges, want=[0] * len(ranges))


def check_random_ranges(eng, n=256):
    srcs, images = range_files(8)
    idxs, sts, _ = eng.bgzf_index_batch(images)
    assert sts == [0] * 8
    rng = random.Random(20261019)
    ranges = [(rng.randrange(8), rng.randrange(len(srcs[0]) + 2000), rng.randrange(1, 30000)) for _ in range(n)]
    check_ranges(eng, srcs, images, idxs, ranges, want=[0] * n)


def check_ranges_foreign_members(eng):
    """members another tool made: several deflate blocks each, subfields in front of BC, a marker in the middle"""
    a, c = pattern(5000, 21), noise(900, 23)
    image = flushed_member(a) + bm.EOF + mem(c, extra=subfield(b"XY", b"123")) + flushed_member(a) + bm.EOF
    src = a + c + a
    idx = bm.index(image)[1]
    ranges = [(0, 4990, 20), (0, 0, len(src)), (0, 5000, 900), (0, 4999, 902), (0, 5899, 2)]
    check_ranges(eng, [src], [image], [idx], ranges, want=[0] * len(ranges))


def check_damaged_member(eng):
    """a damaged member fails only the ranges that touch it"""
    srcs, images = range_files(2)
    idx = [bm.index(x)[1] for x in images]
    lo, hi = idx[0][3][0], idx[0][4][0]
    for at, st in (((lo + hi) // 2, None), (hi - 8, bm.CHECKSUM), (hi - 4, bm.INVALID_BUFFER), (lo + 2, bm.UNSUPPORTED_METHOD)):
        bad = bytearray(images[0])
        bad[at] ^= 0x41
        ranges = [(0, 3 * RB + 5, 10), (0, 100, 50), (0, 2 * RB + 1, 3 * RB), (1, 3 * RB + 5, 10), (0, 4 * RB, 100), (0, 0, 3 * RB)]
        outs, sts = check_ranges(eng, srcs, [bytes(bad), images[1]], idx, ranges)
        assert [s != 0 for s in sts] == [True, False, True, False, False, False]
        if st is not None:
            assert sts[0] == sts[2] == st


def check_unsound_indexes(eng):
    """every kind of unsound index, for one image among good ones; ISIZE that disagrees with a sound index"""
    srcs, images = range_files(3)
    idx = [bm.index(x)[1] for x in images]
    good = idx[1]
    ranges = [(0, 10, 10), (1, 10, 10), (2, 5000, 10), (1, 2 * RB, 10), (1, 0, 0), (1, 1 << 40, 4)]
    kinds = [[], [(0, 1)] + good[1:], good[:2] + [(good[1][0] - 1, good[2][1])] + good[3:],
             good[:2] + [(good[2][0], good[1][1] - 1)] + good[3:], [(0, 0), (good[-1][0], 65537)],
             good[:-1] + [(len(images[1]) + 1, good[-1][1])]]
    for bad in kinds:
        assert not bm.index_sound(bad, len(images[1]))
        check_ranges(eng, srcs, images, [idx[0], bad, idx[2]], ranges, want=[0, bm.INVALID_BUFFER, 0] + [bm.INVALID_BUFFER] * 3)
    # None, what bgzf_index_batch returns for an image that failed, is an index of no entries
    outs, sts = eng.bgzf_read_ranges(images, [idx[0], None, idx[2]], ranges)
    assert sts == [0, bm.INVALID_BUFFER, 0] + [bm.INVALID_BUFFER] * 3 and outs[0] == srcs[0][10:20]
    # sound, but not this file's: uoff of one entry moved, coff of one entry moved
    moved_u = good[:2] + [(good[2][0], good[2][1] - 1)] + good[3:]
    moved_c = good[:2] + [(good[2][0] + 1, good[2][1])] + good[3:]
    only = [bm.index_sound(m, len(images[1])) for m in (moved_u, moved_c)]
    assert only == [True, True]
    for m in (moved_u, moved_c):
        rr = [(1, RB + 5, 10), (1, 2 * RB + 5, 10), (1, 5, 10), (1, 3 * RB + 5, 10), (0, 5, 10)]
        outs, sts = check_ranges(eng, None, images, [idx[0], m, idx[2]], rr)
        assert sts[0] == bm.INVALID_BUFFER and sts[1] != 0 and sts[2:] == [0, 0, 0]
        assert outs[2] == srcs[1][5:15] and outs[3] == srcs[1][3 * RB + 5:3 * RB + 15]


def check_range_call_errors(eng):
    srcs, images = range_files(1)
    idx = [bm.index(x)[1] for x in images]
    with pytest.raises(ZippyError) as e:
        eng.bgzf_read_ranges(images, idx, [(0, 0, 1), (1, 0, 1)])
    assert e.value.status == bm.ARGUMENT


def check_api(eng, api):
    src = pattern(3 * 65280 + 5, 90)
    image = api.bgzf_compress(src, 1)
    assert image == written(src, 1, 0) and api.bgzf_uncompress(image) == src
    idx = api.bgzf_index(image)
    assert idx == bm.index(image)[1]
    assert api.bgzf_read_range(image, idx, 65270, 100) == src[65270:65370]
    assert api.bgzf_read_range(image, idx, len(src) + 1, 100) == b""
    bad = bytearray(image)
    bad[idx[1][0] - 8] ^= 1  # the first member's CRC
    with pytest.raises(ZippyError) as e:
        api.bgzf_read_range(bytes(bad), idx, 5, 100)
    assert e.value.status == bm.CHECKSUM
    with pytest.raises(ZippyError):
        api.bgzf_uncompress(bytes(bad))
    with pytest.raises(ZippyError):
        api.bgzf_index(image[:-5])
    outs, sts = api.bgzf_read_ranges([bytes(bad)], [idx], [(0, 5, 100), (0, 65280, 100)])
    assert sts == [bm.CHECKSUM, 0] and outs == [None, src[65280:65380]]
    outs, sts = api.bgzf_compress_batch([src[:10], b""], 1, 7)
    assert api.bgzf_uncompress_batch(outs) == ([src[:10], b""], [0, 0])


# ---------------------------------------------------------------------------
# the cases as files, for tests/bgzf_sanitize_main.cpp
# ---------------------------------------------------------------------------
def _flagging_decoder(flag):
    def decode(cdata):
        st, out = bm.oracle_decoder(cdata)
        if st != bm.OK:
            flag.append(st)
        return st, out
    return decode


def dump(path):
    """-> the number of (files written, images to read, ranges)"""
    import os
    os.makedirs(path)

    def put(name, data):
        with open(os.path.join(path, name), "wb") as f:
            f.write(data)

    def put_index(name, idx):
        put(name, "".join("%d %d\n" % e for e in (idx or [])).encode())

    lines, read_lines = [], []
    for level, b in ((1, 7), (6, 7), (-2, 4096), (0, 4096), (1, 4096), (9, 4096), (1, 0), (-2, 65505)):
        srcs = [pattern(n, 1 + i) for i, n in enumerate(lengths(b or 65280))] if b != 65505 else list(fallback_pair())
        for i, src in enumerate(srcs):
            name = "w_%d_%d_%d" % (level + 2, b, i)
            image = written(src, level, b)
            put(name + ".src", src)
            put(name + ".bgzf", image)
            lines.append("%s %d %d" % (name, level, b))
            put(name + ".out", src)  # everything written is read and indexed too
            put_index(name + ".idx", bm.index(image)[1])
            read_lines.append("%s 0 1" % name)
    put("write.txt", "\n".join(lines).encode())
    n_write = len(lines)

    pair, pair_want = straddling_pair()
    images = [(image, None) for _, image, _ in good_images()] + [(many_members()[0], None)]
    images += [(image, None) for _, image, _ in bad_images()] + [(x, None) for x in pair]
    lines = read_lines
    for i, (image, _) in enumerate(images):
        flag = []
        st, data, eof = bm.read(image, _flagging_decoder(flag))
        name = "r_%d" % i
        put(name + ".bgzf", image)
        if st == bm.OK:
            put(name + ".out", data)
        put_index(name + ".idx", bm.index(image)[1])
        lines.append("%s %d %d" % (name, -1 if flag else st, eof))
    put("expected.txt", "\n".join(lines).encode())
    n_read = len(lines)

    srcs, files = range_files(3)
    idx = [bm.index(x)[1] for x in files]
    damaged = bytearray(files[1])
    damaged[idx[1][4][0] - 8] ^= 1  # the CRC of member 3
    unsound = idx[2][:2] + [(idx[2][1][0] - 1, idx[2][2][1])] + idx[2][3:]
    names = []
    for i, (image, index) in enumerate(((files[0], idx[0]), (bytes(damaged), idx[1]), (files[2], unsound))):
        put("g_%d.bgzf" % i, image)
        put("g_%d.src" % i, srcs[i])
        put_index("g_%d.idx" % i, index)
        names.append("g_%d" % i)
    put("images.txt", "\n".join(names).encode())
    rng = random.Random(77)
    ranges = [(0, RB + 100 + a, 2 * RB - 300 + 17 * a) for a in range(16)]
    ranges += [(rng.randrange(3), rng.randrange(len(srcs[0]) + 500), rng.randrange(0, 20000)) for _ in range(48)]
    ranges += [(0, 0, 1 << 62), (1, 3 * RB + 1, 1), (1, 0, 3 * RB), (2, 0, 0), (0, 1 << 50, 3)]
    outs, sts = bm.ranges([files[0], bytes(damaged), files[2]], [idx[0], idx[1], unsound], ranges)
    assert bm.CHECKSUM in sts and bm.INVALID_BUFFER in sts and sts.count(0) > 20
    put("ranges.txt", "\n".join("%d %d %d %d" % (t, off, n, st) for (t, off, n), st in zip(ranges, sts)).encode())
    return n_write, n_read, len(ranges)
