"""CPU-only: the model of the resumable uncompress (tests/resume_model.py) against zlib.decompressobj -- the
concatenated output of a chain of calls, at any chunking -- and against tests/seek_model.py: the boundaries it stops at
are the block starts that model reports."""
import random
import zlib

import pytest

import resume_cases as rc
import resume_model as rm
import seek_cases as sc
import seek_model as sm

WBITS_OF = {rm.DF_DEFLATE: -15, rm.DF_ZLIB: 15, rm.DF_GZIP: 31}


def feed(z, piece, max_out, fmt, last_at_end=True):
    """-> (output, states after every call, the bytes left behind the trailer)"""
    state, buf, pos, out, states = None, b"", 0, [], []
    why = rm.NEED_INPUT
    while why != rm.DONE:
        if why == rm.NEED_INPUT:
            assert pos < len(z)
            buf += z[pos:pos + piece]
            pos += piece
        o, used, state, why, st = rm.step(state, buf, max_out, last_at_end and pos >= len(z), fmt)
        assert st == rm.OK, st
        if why == rm.NEED_OUTPUT and not o:
            max_out *= 2
        out.append(o)
        buf = buf[used:]
        states.append(state)
    return b"".join(out), states, buf + z[pos:]


@pytest.mark.parametrize("fmt", rc.FORMATS)
def test_model_small_stream_any_chunking(fmt):
    z, plain = rc.small(fmt)
    assert zlib.decompressobj(WBITS_OF[fmt]).decompress(z) == plain
    for piece, max_out in ((1, rc.BIG), (61, rc.BIG), (61, 700), (1000, 333), (len(z), rc.BIG)):
        out, states, left = feed(z, piece, max_out, fmt)
        assert out == plain and left == b"" and states[-1] is None
        assert all(rm.sound(s) for s in states[:-1] if s is not None)


def test_model_boundaries_are_seek_models_block_starts():
    raw, plain = rc.small_raw()
    _, blocks, end_bit = sm.inflate(raw)
    out, bit, why, st, marks = rm.decode(raw, 0, b"", rc.BIG, False)
    assert (out, bit, why, st) == (plain, end_bit, rm.DONE, rm.OK) and marks == blocks + [(end_bit, len(plain))]
    # every state of a chain stands at one of them, with the window and the checksum of the bytes before it
    z, _ = rc.small(rm.DF_GZIP)
    body = sm.body_bit(z, sm.DF_GZIP)
    starts = {b + body: o for b, o in blocks}
    _, states, _ = feed(z, 97, 500, rm.DF_DETECT)
    for blob in states[:-1]:
        s = rm.State(blob)
        if s.phase == 2:
            assert s.total_out == len(plain) and s.bit_skip == 0
            continue
        assert starts[8 * s.total_in + s.bit_skip] == s.total_out
        assert s.window == plain[:s.total_out][-rm.WINDOW:] and s.check == zlib.crc32(plain[:s.total_out])


def test_model_walk_changes_nothing():
    """decode() may start at a boundary of a Walk of the same stream: the answers are those without it, for first calls
    at any cut and for the second calls behind them, on sound and on damaged hand-built streams"""
    rng = random.Random(2)
    cases = sc.parity_crafted(True)
    walks = rc.crafted_walks(True)
    n = 0
    for (name, raw, plain, _), walk in zip(cases, walks):
        cuts = {len(raw) // 2, len(raw)} | {min(len(raw), b // 8) for b in walk.bits[1:]}
        for cut in sorted(cuts) if len(cuts) < 12 else rng.sample(sorted(cuts), 12):
            for max_out in (1 << 30, 100):
                a = rm.step(None, raw[:cut], max_out, False, rm.DF_DEFLATE, None, walk)
                assert a == rm.step(None, raw[:cut], max_out, False, rm.DF_DEFLATE), (name, cut)
                if a[4] == rm.OK and a[2] is not None:
                    b = rm.step(a[2], raw[a[1]:], max_out, True, rm.DF_DEFLATE, None, walk)
                    assert b == rm.step(a[2], raw[a[1]:], max_out, True, rm.DF_DEFLATE), (name, cut)
                    n += 1
    assert n > 400


def test_model_mix_against_zlib():
    plain = sc.mix()
    z = sc.deflate(plain, 6, 15, 8)
    out, states, left = feed(z + b"tail", 70001, 50000, rm.DF_ZLIB, last_at_end=False)
    assert out == plain and left == b"tail"
    s = rm.State(states[3])
    assert s.win_len == rm.WINDOW and s.check == zlib.adler32(plain[:s.total_out])


def test_model_checksums_and_static_rules():
    rng = random.Random(1)
    blob = bytes(rng.randrange(256) for _ in range(10000))
    assert rm.crc32(blob[4000:], rm.crc32(blob[:4000])) == zlib.crc32(blob)
    assert rm.adler32(blob[4000:], rm.adler32(blob[:4000])) == zlib.adler32(blob)
    z, _ = rc.small(rm.DF_ZLIB)
    state = rm.step(None, z[:1200], rc.BIG)[2]
    assert rm.sound(state) and len(rc.damaged_states(state)) == 17
    assert rm.step(rc.damaged_states(state)[0], z[1200:], rc.BIG)[4] == rm.INVALID_BUFFER
