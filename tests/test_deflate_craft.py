"""The hand-built deflate streams of parity_cases.crafted_streams() (tests/deflate_craft.py) on the CPU, before any
device sees them: the oracle makes of every stream what the builder says it is -- the bytes, or a rejection with the
status of the one fault planted --, zlib gives the same bytes wherever it takes the stream, and the streams cover the
bit phases they are built to cover."""
import zlib

import deflate_craft as dc
import oracle
import parity_cases as pc

# What the reference accepts and zlib refuses: its code tables only reject over-subscription (inflate.nim:24-65), so
# incomplete codes pass as long as no unused pattern turns up.  Nothing joins this set unnoticed.
ORACLE_ONLY = {
    "T2/lit_short_used", "T2/lit_long_used", "T2/dist_short_used", "T2/dist_long_used",
    "H3/single_symbol",
}


def _oracle(blob):
    try:
        return oracle.uncompress(blob, oracle.dfDeflate), None
    except oracle.ZippyError as e:
        return None, e.status


def _zlib(blob):
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(blob)
    except zlib.error:
        return None
    return out if d.eof else None


def test_builder_against_zlib_streams():
    """the builder's own tables: a stream restated token by token from a text decodes to it"""
    s = dc.Stream()
    text = b"a man a plan a canal panama " * 40
    s.fixed_block(False)
    for b in text[:28]:
        s.lit(b)
    s.match(258, 28), s.match(100, 28), s.eob()
    s.stored(b"stored", False, pad_bits=0x55)
    lit, dist = pc._t1_code()
    s.dynamic_block(lit, dist, True, {"symbols": dc.rle_plain(lit + dist)})
    s.match(258, 100, length_symbol=284), s.lit(0), s.lit(255), s.eob()
    blob, plain, status = s.finish()
    want = bytearray(text[:386] + b"stored")
    for _ in range(258):
        want.append(want[-100])
    assert status is None and plain == bytes(want) + b"\x00\xff"
    assert zlib.decompress(blob, -15) == plain and oracle.uncompress(blob, oracle.dfDeflate) == plain


def test_crafted_streams_are_what_the_builder_says():
    info = {}
    cases = pc.crafted_streams(False, info)
    assert len({c[0] for c in cases}) == len(cases)
    counts = {}
    oracle_only = set()
    for name, blob, plain, status in cases:
        counts[name.split("/")[0]] = counts.get(name.split("/")[0], 0) + 1
        assert (plain is None) == (status is not None), name
        got, st = _oracle(blob)
        assert got == plain, (name, "oracle status", st, "length", None if got is None else len(got))
        assert st == status, (name, st, status)
        z = _zlib(blob)
        if z is not None:
            assert z == plain, (name, "zlib")
        elif plain is not None:
            oracle_only.add(name)
    assert counts == pc.CRAFT_COUNTS
    assert oracle_only == ORACLE_ONLY
    tok48, fixed, dynamic = pc.crafted_coverage(info)
    assert len(tok48) == 512 and len(fixed) == 512 and len(dynamic) == 512
    assert sum(len(c[2]) for c in cases if c[2] is not None) < 4 << 20


def test_crafted_streams_small_subset():
    info = {}
    cases = pc.crafted_streams(True, info)
    full = {c[0]: c for c in pc.crafted_streams(False)}
    counts = {}
    for name, blob, plain, status in cases:
        counts[name.split("/")[0]] = counts.get(name.split("/")[0], 0) + 1
        got, st = _oracle(blob)
        assert (got, st) == (plain, status), name
        if status is not None:
            assert full[name][3] == status
    assert counts == pc.CRAFT_COUNTS_SMALL
    tok48, fixed, dynamic = pc.crafted_coverage(info)
    assert len(tok48) == 512 and len(fixed) == 512 and len(dynamic) == 512
    assert sum(1 for p, bits, kind in info["T1/48_bit_tokens"][0]) <= 601
    assert sum(len(c[2]) for c in cases if c[2] is not None) < 600000


def test_reader_against_zlib_and_oracle_streams():
    """deflate_craft.read_blocks, the reader the parallel parse's streams are held against (check_l1p_streams): what
    its tokens replay to is what zlib.decompressobj makes of streams zlib and the oracle wrote -- stored, fixed and
    dynamic blocks, several blocks a stream --, and it reads the builder's own tokens and code lengths back"""
    import random
    import synth
    alice, html = synth.corpus_file("alice29.txt"), synth.corpus_file("html")
    plains = [alice[:70000], html[:40000], b"", b"a", b"\x00" * 70000, random.Random(9).randbytes(3000), b"ab" * 20000,
              alice[:300]]
    streams = []
    for plain in plains:
        for level, strategy in ((1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_FIXED), (0, zlib.Z_DEFAULT_STRATEGY)):
            co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
            streams.append((co.compress(plain[:len(plain) // 2]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(plain[len(plain) // 2:]) +
                            co.flush(), plain))
        for level in (1, -1, -2, 0):
            streams.append((oracle.compress(plain, level, oracle.dfDeflate), plain))
    types = set()
    for raw, plain in streams:
        d = zlib.decompressobj(-15)
        want = d.decompress(raw)
        assert d.eof and want == plain
        blocks = dc.read_blocks(raw)
        assert dc.replay(blocks) == want
        assert blocks[-1]["final"] and not any(b["final"] for b in blocks[:-1])
        types |= {b["type"] for b in blocks}
        for b in blocks:
            if b["type"] == 2:
                assert 257 <= len(b["lit_lens"]) <= 286 and 1 <= len(b["dist_lens"]) <= 30 and b["lit_lens"][256]
                assert dc.kraft(b["lit_lens"]) <= 32768 and dc.kraft(b["dist_lens"]) <= 32768
    assert types == {0, 1, 2}
    # the builder's own: tokens and code lengths come back as written
    s = dc.Stream()
    lit, dist = pc._t1_code()
    s.stored(bytes(range(120)), False, pad_bits=0x0a)
    s.dynamic_block(lit, dist, False, {"symbols": dc.rle_plain(lit + dist)})
    s.lit(0), s.lit(255), s.match(5, 2), s.match(3, 1), s.match(258, 100, length_symbol=284), s.eob()
    s.fixed_block(True)
    s.lit(65), s.match(4, 1), s.match(258, 5), s.eob()
    raw, plain, status = s.finish()
    assert status is None
    blocks = dc.read_blocks(raw)
    assert [b["type"] for b in blocks] == [0, 2, 1] and dc.replay(blocks) == plain
    assert blocks[0]["tokens"] == [("lit", b) for b in range(120)]
    assert blocks[1]["lit_lens"] == list(lit) and blocks[1]["dist_lens"] == list(dist)
    assert blocks[1]["tokens"] == [("lit", 0), ("lit", 255), ("match", 5, 2), ("match", 3, 1), ("match", 258, 100)]
    assert blocks[2]["tokens"] == [("lit", 65), ("match", 4, 1), ("match", 258, 5)]
    assert blocks[2]["lit_lens"] == dc.FIXED_LIT_LENS and blocks[2]["dist_lens"] == dc.FIXED_DIST_LENS
