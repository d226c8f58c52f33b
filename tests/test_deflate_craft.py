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
