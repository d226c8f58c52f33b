"""Cases of zh_seek_index_batch / zh_seek_read_ranges shared by tests/test_emu_seek.py (fiber emulator),
tests/test_gpu_seek.py (MI355X) and, dumped, tests/test_seek_sanitize.py.  Streams come from Python's zlib over
synth.py's data, from the engine's own compress / compress_blocks and from tests/deflate_craft.py; the expected blob
is the model's (tests/seek_model.py), byte for byte; a range's expected bytes are the slice of the original input."""
import functools
import os
import random
import struct
import zlib

import pytest

import deflate_craft as dc
import seek_model as sm
import synth
from zippy_amd.common import ZippyError

OK, INVALID_BUFFER, CHECKSUM, ARGUMENT = 0, 13, 8, 22
M64 = (1 << 64) - 1
SPAN = 32768
FAMILY = ((6, 8), (6, 1), (1, 1), (9, 4))               # (level, memLevel)
WBITS = ((-15, sm.DF_DEFLATE), (31, sm.DF_GZIP), (15, sm.DF_ZLIB))
FAMILY_POINTS = (3, 11, 11, 9)                          # points before the closing entry (raw deflate: 3, 383, 628, 47 blocks)


def deflate(src, level, wbits, mem, flush_every=0, flush=zlib.Z_SYNC_FLUSH):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, mem)
    if not flush_every:
        return c.compress(src) + c.flush()
    out = b""
    for o in range(0, len(src), flush_every):
        out += c.compress(src[o:o + flush_every]) + c.flush(flush)
    return out + c.flush()


@functools.lru_cache(maxsize=None)
def mix(size=327680 + 12345, index=7):
    return synth.gen_mix_buffer(index, size).tobytes()


@functools.lru_cache(maxsize=None)
def family(wbits):
    """the four streams of the first build family in one container"""
    return [deflate(mix(), lv, wbits, mem) for lv, mem in FAMILY]


@functools.lru_cache(maxsize=None)
def model(data, fmt, span=SPAN):
    """(blob, plaintext) by the model, made once a stream"""
    return sm.build_index(data, fmt, span)


def build(eng, streams, fmt, span, want_data=True):
    out = eng.seek_index_batch(streams, fmt, span, want_data=want_data)
    assert all(len(x) == len(streams) for x in out)
    return out


def check_build(eng, streams, fmt, span, want_data=True):
    """every stream is sound: blob and data equal the model's"""
    out = build(eng, streams, fmt, span, want_data)
    for i, data in enumerate(streams):
        blob, plain = model(data, sm.resolve_format(data, fmt), span or sm.DEFAULT_SPAN)
        assert out[1][i] == OK, (i, out[1][i])
        assert out[0][i] == blob, (i, sm.Blob(out[0][i]).points[:3], sm.Blob(blob).points[:3])
        if want_data:
            assert out[2][i] == plain, i
    return out[0]


# ---- build ----
def check_build_family(eng):
    for wbits, fmt in WBITS:
        blobs = check_build(eng, family(wbits), fmt, SPAN)
        assert tuple(sm.Blob(b).n_points - 1 for b in blobs) == FAMILY_POINTS
        if fmt == sm.DF_GZIP:  # (the bit offsets include the container's header)
            assert sm.Blob(blobs[0]).points[0][0] == 80
    # ... and the containers told apart by the library, the data not asked for
    check_build(eng, family(31) + family(15), sm.DF_DETECT, SPAN, want_data=False)


def check_build_spans(eng):
    data = family(31)[1]
    two = check_build(eng, [data], sm.DF_GZIP, 1 << 20)[0]
    assert sm.Blob(two).n_points == 2
    assert check_build(eng, [data], sm.DF_GZIP, 0, want_data=False)[0] == two  # (0: 1 MiB)
    for span in (1, 32767):
        with pytest.raises(ZippyError) as e:
            eng.seek_index_batch([data], sm.DF_GZIP, span)
        assert e.value.status == ARGUMENT
    blobs, sts = eng.seek_index_batch([], sm.DF_GZIP, 0)
    assert (blobs, sts) == ([], [])


def flushed_streams():
    src = mix()[:150000]
    return [(deflate(src, 6, 31, 8, 20000, zlib.Z_SYNC_FLUSH), sm.DF_GZIP),
            (deflate(src, 6, 15, 8, 9000, zlib.Z_FULL_FLUSH), sm.DF_ZLIB),
            (deflate(src[:70000], 6, -15, 8, 35000), sm.DF_DEFLATE)]


def double_flush():
    """flushes in a row: several boundaries at one out_off, the first that qualifies is the point"""
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    src = mix()[:100000]
    out = c.compress(src[:40000]) + c.flush(zlib.Z_SYNC_FLUSH) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(src[40000:])
    out += c.flush(zlib.Z_SYNC_FLUSH) + c.flush(zlib.Z_SYNC_FLUSH)
    return out + c.flush()


def check_build_small_and_own(eng):
    check_build(eng, [deflate(b"", 6, 31, 8)], sm.DF_GZIP, SPAN)
    src = mix()[:200000]
    own = eng.compress(src, 1, sm.DF_GZIP)
    assert sm.Blob(check_build(eng, [own], sm.DF_GZIP, SPAN)[0]).n_points == 2  # (one block)
    blocks, idx = eng.compress_blocks(src, 1, sm.DF_ZLIB, 32768)
    b = sm.Blob(check_build(eng, [blocks], sm.DF_ZLIB, SPAN)[0])
    assert [tuple(p[:2]) for p in b.points][:-1] == [tuple(e) for e in idx][:-1]  # (a point at every block)
    assert b.points[-1][1] == idx[-1][1]
    for data, fmt in flushed_streams():
        check_build(eng, [data], fmt, SPAN)
    data = double_flush()
    _, blocks_seen, _ = sm.inflate(data, 0)
    outs = [b[1] for b in blocks_seen]
    assert len(outs) - len(set(outs)) >= 3  # (boundaries that share an out_off)
    check_build(eng, [data], sm.DF_DEFLATE, SPAN)


def _lits(s, data):
    for b in data:
        s.lit(b)


def crafted():
    """[(raw deflate, plaintext)]: a stored block entered at each of the 8 bit alignments right at a point; a match of
    distance 32768 as the first token behind a point; a fixed-Huffman block as a point's first block"""
    out = []
    filler = mix()[1000:1000 + SPAN]
    for phase in range(8):
        s = dc.Stream()
        s.stored(filler[:SPAN - 200], False)
        s.fixed_block(False)
        _lits(s, filler[SPAN - 200:])
        # (literals of 8 or 9 bits and the 7-bit end of block: trim until the next header sits at the wanted phase)
        extra = 0
        while (s.bitpos + 7) % 8 != phase:
            s.lit(0x90 + extra)  # a 9-bit literal moves the phase by one
            extra += 1
        s.eob()
        assert s.bitpos % 8 == phase
        s.stored(b"stored behind a point, phase %d " % phase * 40, False, pad_bits=0x55)
        s.fixed_block(True)
        _lits(s, b"the end")
        s.eob()
        raw, plain, status = s.finish()
        assert status is None
        out.append((raw, plain))
    s = dc.Stream()
    s.stored(filler, False)
    s.fixed_block(True)  # a point's first block, and its first token reaches the window's first byte
    s.match(258, 32768)
    s.match(3, 32768)
    _lits(s, b"tail")
    s.eob()
    raw, plain, status = s.finish()
    assert status is None
    out.append((raw, plain))
    return out


def check_build_crafted(eng):
    cases = crafted()
    blobs = check_build(eng, [raw for raw, _ in cases], sm.DF_DEFLATE, SPAN)
    phases = set()
    for (raw, plain), blob in zip(cases, blobs):
        b = sm.Blob(blob)
        assert model(raw, sm.DF_DEFLATE)[1] == plain and b.n_points == 3
        phases.add(b.points[1][0] % 8)
        ranges = [(0, b.points[1][1] - 1, 300), (0, b.points[1][1], 258), (0, 0, len(plain))]
        check_read(eng, [plain], [raw], [blob], ranges)
    assert phases == set(range(8))


@functools.lru_cache(maxsize=None)
def zeros_stream():
    """1 MiB of zeros: a thousand-fold expansion with a point about every block -- the point lists' capacity"""
    for mem in (1, 2, 3):
        data = deflate(bytes(1 << 20), 6, 15, mem)
        if sm.Blob(model(data, sm.DF_ZLIB)[0]).n_points - 1 >= 16:
            return data
    raise AssertionError("no memLevel gives 16 points")


def check_build_zeros(eng):
    data = zeros_stream()
    assert len(data) * 700 < (1 << 20)
    blob = check_build(eng, [data], sm.DF_ZLIB, SPAN, want_data=False)[0]
    b = sm.Blob(blob)
    check_read(eng, [bytes(1 << 20)], [data], [blob], [(0, b.points[5][1] - 1, 2), (0, (1 << 20) - 3, 100)])


def check_build_list_retry(eng, monkeypatch, capfd):
    """point lists too short for the stream (a first attempt of 4 entries a list): counted, decoded once more, same blob"""
    monkeypatch.setenv("ZH_SEEK_FIRST_CAP", "4")
    monkeypatch.setenv("ZH_TRACE", "1")
    check_build(eng, [family(-15)[1], deflate(mix()[:50000], 6, -15, 8)], sm.DF_DEFLATE, SPAN)
    assert "point lists cut short" in capfd.readouterr().err


@functools.lru_cache(maxsize=None)
def batch33():
    """33 streams of both detectable containers; 5 has a damaged CRC trailer, 20 is truncated -> (streams, sources)"""
    streams, srcs = [], []
    for i in range(33):
        src = mix(70000 + 37 * i, 100 + i)
        lv, mem = FAMILY[i % 4]
        streams.append(deflate(src, lv, 31 if i % 3 else 15, mem))
        srcs.append(src)
    bad = bytearray(streams[5])
    bad[-6] ^= 0x40  # (stream 5 is gzip: its CRC-32)
    streams[5] = bytes(bad)
    streams[20] = streams[20][:len(streams[20]) * 2 // 3]
    return streams, srcs


def check_build_batch33(eng):
    streams, srcs = batch33()
    blobs, sts, outs = build(eng, streams, sm.DF_DETECT, SPAN)
    _, want_sts = eng.uncompress_batch(streams, sm.DF_DETECT)
    assert sts == want_sts and sts[5] != OK and sts[20] != OK and sts.count(OK) == 31
    for i in range(33):
        if i in (5, 20):
            assert blobs[i] is None and outs[i] is None
        else:
            assert blobs[i] == model(streams[i], sm.DF_DETECT)[0] and outs[i] == srcs[i], i
    return blobs


# ---- read ----
def want_slice(src, off, length):
    return src[off:off + length] if off < len(src) else b""


def check_read(eng, srcs, streams, blobs, ranges, bad=None):
    """One call: every range not in `bad` returns its slice with ZH_OK; bad: {range: status, or -1 for any status but
    ZH_OK and ZH_ERR_CHECKSUM}.  -> (outs, statuses)"""
    bad = bad or {}
    outs, sts = eng.seek_read_ranges(streams, blobs, ranges)
    assert len(outs) == len(sts) == len(ranges)
    for r, (s, off, length) in enumerate(ranges):
        if r in bad:
            assert outs[r] is None, r
            assert sts[r] == bad[r] if bad[r] >= 0 else sts[r] not in (OK, CHECKSUM), (r, ranges[r], sts[r], bad[r])
        else:
            assert sts[r] == OK, (r, ranges[r], sts[r])
            assert outs[r] == want_slice(srcs[s], off, length), (r, ranges[r])
    return outs, sts


def stream_ranges(s, blob, total):
    """the read cases of one stream"""
    b = sm.Blob(blob)
    offs = [p[1] for p in b.points]
    out = [(s, 0, total), (s, 0, 1), (s, total - 1, 1)]
    out += [(s, o - 1, 2) for o in offs[1:]]                    # straddling two intervals
    out += [(s, offs[1] + 10, 100)]                             # strictly inside one
    out += [(s, offs[1], offs[min(4, len(offs) - 1)] - offs[1])]  # from one point to the point three further on
    out += [(s, total, 10), (s, total + 12345, 10), (s, 5, 0), (s, 5, M64), (s, total - 2, M64 - 1)]
    return out


def check_read_family(eng, wbits_fmt=WBITS):
    for wbits, fmt in wbits_fmt:
        streams = family(wbits)
        blobs = [model(d, fmt)[0] for d in streams]
        ranges = [r for s in range(len(streams)) for r in stream_ranges(s, blobs[s], len(mix()))]
        check_read(eng, [mix()] * len(streams), streams, blobs, ranges)
        up, in_place, via = eng.debug_range_stats()
        assert up == sm.upload_bytes([sm.Blob(b) for b in blobs], [len(d) for d in streams], ranges)
        assert in_place == 0 and via == sum(len(sm.Blob(blobs[s]).touched(o, n)) for s, o, n in ranges)


def check_read_batch33(eng, blobs):
    streams, srcs = batch33()
    rng = random.Random(33)
    ranges = []
    for s in range(33):
        n = len(srcs[s])
        ranges += [(s, rng.randrange(n), rng.randrange(1, 40000)) for _ in range(3)] + [(s, 32767, 3)]
    rng.shuffle(ranges)
    bad = {r: INVALID_BUFFER for r, q in enumerate(ranges) if q[0] in (5, 20)}  # (no blob: a blob of no bytes)
    check_read(eng, srcs, streams, blobs, ranges, bad)


def check_upload_accounting(eng):
    data = family(31)[1]
    blob = model(data, sm.DF_GZIP)[0]
    b = sm.Blob(blob)
    one = [(0, b.points[4][1] + 5, 1000)]
    check_read(eng, [mix()], [data], [blob], one)
    up, _, via = eng.debug_range_stats()
    assert via == 1 and up == sm.upload_bytes([b], [len(data)], one)
    assert up < len(data) // 5 + 32768  # a one-interval range: a fraction of the stream, and a window
    # overlapping and touching spans and windows are sent once; two ranges that share an interval decode it twice
    many = [(0, b.points[2][1] + 5, 10), (0, b.points[2][1] + 50, 40000), (0, b.points[3][1] - 1, 2),
            (0, b.points[7][1], 10), (0, 0, 5)]
    check_read(eng, [mix()], [data], [blob], many)
    up, _, via = eng.debug_range_stats()
    assert via == sum(len(b.touched(o, n)) for _, o, n in many) == 7 and up == sm.upload_bytes([b], [len(data)], many)


def check_scratch_groups(eng, monkeypatch, capfd):
    """a scratch budget of 1 MiB: groups of ranges take turns and return the same bytes"""
    data = family(-15)[3]
    blob = model(data, sm.DF_DEFLATE)[0]
    ranges = [(0, p[1] - 1, 2) for p in sm.Blob(blob).points[1:-1]] * 3  # 24 ranges of two slots of 32 + 32 KiB and more
    want = check_read(eng, [mix()], [data], [blob], ranges)
    monkeypatch.setenv("ZH_SCRATCH_MB", "1")
    monkeypatch.setenv("ZH_TRACE", "1")
    capfd.readouterr()
    assert check_read(eng, [mix()], [data], [blob], ranges) == want
    assert "seek scratch for" in capfd.readouterr().err


# ---- damage ----
def inner_bytes(b, k):
    """the bytes strictly inside interval k's compressed span (none shares a bit with a neighbour)"""
    return range(b.points[k][0] // 8 + 1, b.points[k + 1][0] // 8)


def damage_plan(data, blob, seed0):
    """16 seeded (interval, byte) whose flip the model sees, at most 2 of them without effect -> [(k, at, status)]"""
    b = sm.Blob(blob)
    for seed in range(seed0, seed0 + 50):
        rng = random.Random(seed)
        plan = []
        for _ in range(16):
            k = rng.randrange(b.n_points - 1)
            at = rng.choice(inner_bytes(b, k))
            bad = bytearray(data)
            bad[at] ^= 0xff
            plan.append((k, at, sm.decode_interval(bytes(bad), b, k)[0]))
        if sum(st == OK for _, _, st in plan) <= 2:
            return plan
    raise AssertionError("no seed within 50")


def neighbour_ranges(s, b, k):
    """ranges around interval k of stream s -> (ranges, the positions of those that touch k)"""
    offs = [p[1] for p in b.points]
    assert offs[k + 1] - offs[k] > 7
    ranges, touching = [(s, offs[k] + 7, min(100, offs[k + 1] - offs[k] - 7))], [0]
    if k > 0:
        ranges += [(s, offs[k] - 1, 2), (s, offs[k - 1] + 3, 50)]
        touching.append(1)
    if k + 2 < len(offs):
        ranges += [(s, offs[k + 1] - 1, 2), (s, offs[k + 1] + 3, 50)]
        touching.append(len(ranges) - 2)
    return ranges, touching


def check_damaged_bytes(eng, data, fmt, seed0=1):
    """one call: 16 copies of the stream, each with one byte flipped inside one interval"""
    blob = model(data, fmt)[0]
    b = sm.Blob(blob)
    streams, ranges, bad = [], [], {}
    for k, at, st in damage_plan(data, blob, seed0):
        if st == OK:  # (the model's output is unchanged: nothing to expect)
            continue
        copy = bytearray(data)
        copy[at] ^= 0xff
        rs, touching = neighbour_ranges(len(streams), b, k)
        for t in touching:
            bad[len(ranges) + t] = CHECKSUM if st == CHECKSUM else -1
        ranges += rs
        streams.append(bytes(copy))
    assert len(streams) >= 14
    check_read(eng, [mix()] * len(streams), streams, [blob] * len(streams), ranges, bad)


def check_damaged_window(eng):
    """a flipped window byte: ZH_ERR_CHECKSUM where the interval refers to it, ZH_OK where it does not"""
    data = family(-15)[1]
    blob = model(data, sm.DF_DEFLATE)[0]
    b = sm.Blob(blob)
    rng = random.Random(5)
    blobs, ranges, bad, seen = [], [], {}, set()
    for _ in range(24):
        k = rng.randrange(1, b.n_points - 1)
        p = b.points[k]
        d = sm.Blob(blob)
        store = bytearray(d.store)
        store[p[2] + rng.randrange(p[3])] ^= 0xff
        d.store = bytes(store)
        st = sm.decode_interval(data, d, k)[0]
        assert st in (OK, CHECKSUM)
        seen.add(st)
        rs, touching = neighbour_ranges(len(blobs), b, k)
        if st == CHECKSUM:
            for t in touching:
                bad[len(ranges) + t] = CHECKSUM
        ranges += rs
        blobs.append(d.pack())
    assert seen == {OK, CHECKSUM}
    check_read(eng, [mix()] * len(blobs), [data] * len(blobs), blobs, ranges, bad)


def check_moved_point(eng):
    """bit_off + 1 in one point: the intervals on both sides fail, all others read"""
    data = family(15)[3]
    blob = model(data, sm.DF_ZLIB)[0]
    d = sm.Blob(blob)
    k = 4
    d.points[k][0] += 1
    offs = [p[1] for p in d.points]
    ranges = [(0, offs[j] + 1, 20) for j in range(d.n_points - 1)] + [(0, offs[k - 1] - 1, 2), (0, offs[k + 1] - 1, 2)]
    bad = {k - 1: -1, k: -1, len(ranges) - 2: -1, len(ranges) - 1: -1}
    for j in (k - 1, k):  # (what the model makes of the two)
        assert sm.decode_interval(data, d, j)[0] == INVALID_BUFFER
    check_read(eng, [mix()], [data], [d.pack()], ranges, bad)


def static_damage(blob, src_len):
    """every form of a blob that cannot be right -> [(name, blob)]"""
    def edit(fn):
        d = sm.Blob(blob)
        fn(d)
        return d.pack()

    def setp(k, field, value):
        return lambda d: d.points[k].__setitem__(field, value)

    b = sm.Blob(blob)
    out = [("magic", b"ZHSKIDX2" + blob[8:]),
           ("version", edit(lambda d: setattr(d, "version", 2))),
           ("cut short", blob[:-1]),
           ("one byte more", blob + b"\0"),
           ("a point more than there is", edit(lambda d: setattr(d, "n_points", d.n_points + 1))[:len(blob)]),
           ("window bytes", edit(lambda d: setattr(d, "window_bytes", d.window_bytes + 16))),
           ("header only", blob[:64]),
           ("nothing", b""),
           ("src_len", edit(lambda d: setattr(d, "src_len", src_len + 1))),
           ("out_off[0]", edit(setp(0, 1, 1))),
           ("bit_off not rising", edit(setp(2, 0, b.points[1][0]))),
           ("bit_off beyond the stream", edit(setp(b.n_points - 2, 0, 8 * src_len))),
           ("closing bit_off beyond the stream", edit(setp(b.n_points - 1, 0, 8 * src_len + 1))),
           ("out_off falling", edit(setp(3, 1, b.points[2][1] - 1))),
           ("win_len", edit(setp(2, 3, b.points[2][3] - 1))),
           ("closing win_len", edit(setp(b.n_points - 1, 3, 16))),
           ("window outside the store", edit(setp(2, 2, b.window_bytes - 16))),
           ("window not at a multiple of 16", edit(setp(2, 2, b.points[2][2] + 8)))]

    def too_much(d):
        d.points[-1][1] = d.total = d.points[-2][1] + 1032 * ((d.points[-1][0] + 7) // 8 - d.points[-2][0] // 8) + 65
    out.append(("an interval that promises too much", edit(too_much)))
    return out


def check_static_damage(eng):
    data = family(31)[3]
    blob = model(data, sm.DF_GZIP)[0]
    forms = static_damage(blob, len(data))
    streams = [data] * (len(forms) + 1)
    blobs = [f for _, f in forms] + [blob]
    ranges = [(s, 40000 + s, 100) for s in range(len(streams))] + [(s, 5, 0) for s in range(len(streams))]
    bad = {r: INVALID_BUFFER for r, q in enumerate(ranges) if q[0] < len(forms)}
    check_read(eng, [mix()] * len(streams), streams, blobs, ranges, bad)


def check_call_errors(eng):
    data = family(31)[0]
    blob = model(data, sm.DF_GZIP)[0]
    with pytest.raises(ZippyError) as e:
        eng.seek_read_ranges([data], [blob], [(1, 0, 10)])
    assert e.value.status == ARGUMENT
    assert eng.seek_read_ranges([data], [blob], []) == ([], [])
    assert eng.seek_read_ranges([], [], []) == ([], [])


# ---- points at any block boundary: histories of any length (the engine itself only builds with span >= 32768) ----
def every_block(j, b):
    return True


def one_in_four(seed):
    """a seeded subset: every block start kept with probability 1/4"""
    rng = random.Random(seed)
    return lambda j, b: rng.random() < 0.25


def youngest(data, fmt):
    """the first block and the single block start with the largest out_off below 32768 (none: the first block alone)"""
    blocks = sm.walk(data, sm.resolve_format(data, fmt))[1]
    young = [j for j, b in enumerate(blocks) if j and 0 < b[1] < sm.WINDOW]
    pick = max(young, key=lambda j: (blocks[j][1], -j)) if young else None
    return lambda j, b: j == pick


def dense_streams(small=False):
    """[(stream, format, source)]"""
    out = [(family(-15)[1], sm.DF_DEFLATE, mix()), (double_flush(), sm.DF_DEFLATE, mix()[:100000])]
    if not small:
        out += [(family(15)[2], sm.DF_ZLIB, mix()), (family(31)[3], sm.DF_GZIP, mix())]
        out += [(d, fmt, mix()[:70000 if fmt == sm.DF_DEFLATE else 150000]) for d, fmt in flushed_streams()]
        out += [(zeros_stream(), sm.DF_ZLIB, bytes(1 << 20))]
    return out


def dense_point_sets(small=False):
    """[(name, [blob a stream of dense_streams()])]: every block start, three seeded quarters, the youngest"""
    streams = dense_streams(small)
    sets = [("every block", [every_block] * len(streams))]
    sets += [("a quarter, seed %d" % seed, [one_in_four(1000 * seed + s) for s in range(len(streams))]) for seed in (1, 2, 3)]
    sets += [("the youngest", [youngest(d, fmt) for d, fmt, _ in streams])]
    return [(name, [sm.index_at(d, fmt, keep)[0] for (d, fmt, _), keep in zip(streams, keeps)]) for name, keeps in sets]


def dense_ranges(s, blob):
    """The read cases of one stream under one point set: the whole stream; two bytes across a point at up to 64
    points, every point with a window shorter than 32768 among them; a range strictly inside each of the first four
    intervals; a range across an empty interval where there is one."""
    b = sm.Blob(blob)
    offs = [p[1] for p in b.points]
    out = [(s, 0, b.total)]
    inner = [k for k in range(1, b.n_points - 1) if offs[k] > 0]
    short = [k for k in inner if b.points[k][3] < sm.WINDOW]
    assert len(short) <= 64
    rest = [k for k in inner if b.points[k][3] == sm.WINDOW]
    room = 64 - len(short)
    picked = short + (rest if len(rest) <= room else [rest[(2 * i + 1) * len(rest) // (2 * room)] for i in range(room)])
    out += [(s, offs[k] - 1, 2) for k in sorted(set(picked))]
    for k in range(min(4, b.n_points - 1)):
        if offs[k + 1] - offs[k] >= 3:
            out.append((s, offs[k] + 1, min(100, offs[k + 1] - offs[k] - 2)))
    empty = [k for k in range(1, b.n_points - 1) if offs[k] == offs[k + 1] and 3 <= offs[k] <= b.total - 4]
    if empty:
        out.append((s, offs[empty[0]] - 3, 7))
    return out


def check_dense(eng, small=False):
    """one read call a point set, all streams in it; the bytes, and the upload and the intervals decoded by the model"""
    streams = dense_streams(small)
    for name, blobs in dense_point_sets(small):
        bs = [sm.Blob(b) for b in blobs]
        ranges = [r for s in range(len(streams)) for r in dense_ranges(s, blobs[s])]
        # (... and the short ranges once more in a call of their own: beside a range of the whole stream every span
        # is part of that range's, and the upload says nothing of where a short range's span begins)
        for rs in (ranges, [r for r in ranges if r[2] != bs[r[0]].total]):
            check_read(eng, [src for _, _, src in streams], [d for d, _, _ in streams], blobs, rs)
            up, in_place, via = eng.debug_range_stats()
            assert up == sm.upload_bytes(bs, [len(d) for d, _, _ in streams], rs), name
            assert in_place == 0 and via == sum(len(sm.decoded(bs[s], o, n)) for s, o, n in rs), name


# ---- the hand-built streams of tests/parity_cases.py through both seek kernels ----
HISTORIES = (1, 17, 4097, 32767, 32768)


def parity_crafted(small):
    import parity_cases as pc
    return pc.crafted_streams(small)


def check_crafted_all(eng, small=False):
    """all of them in one build: an accepted stream's blob and data are the model's and the builder's, a rejected one
    has none and the status uncompress_batch gives it in the same batch"""
    cases = parity_crafted(small)
    raws = [c[1] for c in cases]
    blobs, sts, outs = build(eng, raws, sm.DF_DEFLATE, SPAN)
    _, want_sts = eng.uncompress_batch(raws, sm.DF_DEFLATE)
    assert sts == want_sts
    n_good = 0
    for (name, raw, plain, _), blob, st, out in zip(cases, blobs, sts, outs):
        if plain is None:
            assert st != OK and blob is None and out is None, name
            continue
        n_good += 1
        assert st == OK and out == plain, (name, st)
        want_blob, want_plain = model(raw, sm.DF_DEFLATE)
        assert want_plain == plain and blob == want_blob, (name, sm.Blob(blob).points[:3], sm.Blob(want_blob).points[:3])
    assert 0 < n_good < len(cases)
    if not small:  # (the chain of 258-byte matches outgrows the room a raw stream is given: the sizing pass runs)
        big = [c for c in cases if c[0] == "W2/chain_len258_dist1"][0]
        assert len(big[2]) > 4 * len(big[1]) + 65536


def behind_history(small=False):
    """Every accepted crafted stream behind a non-final stored block of H filler bytes (a stored block ends at a byte
    boundary: the concatenation is a stream, its plaintext filler + plaintext) -> [(name, H, stream, plaintext)]"""
    out = []
    good = [c for c in parity_crafted(small) if c[2] is not None]
    for i, (name, raw, plain, _) in enumerate(good):
        h = 4097 if small else HISTORIES[i % len(HISTORIES)]
        filler = mix()[2000 + i:2000 + i + h]
        s = dc.Stream()
        s.stored(filler, False)
        head, _, status = s.finish()
        assert status is None and len(head) == 5 + h
        out.append((name, h, head + raw, filler + plain))
    return out


def check_crafted_behind_history(eng, small=False):
    """indexed at every block start: the crafted body decodes through the seek decoder with a history of min(H, 32768)
    bytes and a stop bit; and the same streams through the build"""
    cases = behind_history(small)
    streams = [c[2] for c in cases]
    blobs = [sm.index_at(d, sm.DF_DEFLATE, every_block)[0] for d in streams]
    ranges = [r for s, (_, h, _, plain) in enumerate(cases) for r in ((s, 0, len(plain)), (s, h - 1, 2), (s, h, 300))]
    check_read(eng, [c[3] for c in cases], streams, blobs, ranges)
    del blobs
    got, sts, outs = build(eng, streams, sm.DF_DEFLATE, SPAN)
    for (name, _, d, plain), blob, st, out in zip(cases, got, sts, outs):
        assert st == OK and out == plain and blob == sm.build_index(d, sm.DF_DEFLATE, SPAN)[0], (name, st)


# ---- a match at, and one past, the window's first byte ----
def edge_code(long_dist=False):
    """A complete dynamic code zlib accepts: every literal, the end of block, lengths 3 and 258, all 30 distances.
    long_dist: the distance codes the cases use are 12 and 13 bits long, beyond the decoders' distance tables (8
    bits) -- such a match is no part of a round, the decode wave hands it over alone."""
    lit = [8] * 254 + [9, 9, 9, 10] + [0] * 27 + [10]
    dist = [4] * 2 + [5] * 28
    if long_dist:
        dist = [12] * 3 + [1, 2, 3, 4, 5, 6, 7, 8] + [12] * 7 + [13] * 12
        assert all(dist[k] > 8 for k in (0, 1, 2, 12, 16, 24, 29))
    assert len(lit) == 286 and len(dist) == 30 and dc.kraft(lit) == 32768 and dc.kraft(dist) == 32768
    return lit, dist


@functools.lru_cache(maxsize=None)
def window_edge_cases():
    """A stored block of P bytes, then one final block of j literals and a match of distance P + j -- it reaches output
    byte 0 --, a literal and the end of block; the final block fixed, dynamic, and dynamic with distance codes too long
    for the decoders' tables -> [(name, P, stream, plaintext)]"""
    out = []
    filler = mix()[5000:5000 + SPAN]
    for kind in ("fixed", "dynamic", "long distance codes"):
        for p in (1, 2, 258, 4097, 32767, 32768):
            for j in (0, 1, 70):
                if p + j > 32768:
                    continue
                for length in (3, 258):
                    s = dc.Stream()
                    s.stored(filler[:p], False)
                    if kind == "fixed":
                        s.fixed_block(True)
                    else:
                        s.dynamic_block(*edge_code(kind != "dynamic"), True)
                    _lits(s, bytes((7 * i + 3) & 0xff for i in range(j)))
                    s.match(length, p + j)
                    s.lit(0x21)
                    s.eob()
                    raw, plain, status = s.finish()
                    assert status is None and len(plain) == p + j + length + 1
                    out.append(("%s P=%d j=%d len=%d" % (kind, p, j, length), p, raw, plain))
    assert len(out) == 90
    return out


def honest_blob(raw):
    return sm.index_at(raw, sm.DF_DEFLATE, every_block)[0]


def forged_past(raw):
    """Every out_off behind point 0 lowered by one, the plaintext without its first byte: it passes every static rule;
    interval 1 has a window of min(P, 32768) - 1 bytes, and its match reaches one byte beyond it; interval 0 makes one
    byte more than promised."""
    plain, blocks, end_bit = sm.walk(raw, sm.DF_DEFLATE)
    assert len(blocks) == 2
    points = [blocks[0], (blocks[1][0], blocks[1][1] - 1), (end_bit, len(plain) - 1)]
    return sm.write_blob(sm.DF_DEFLATE, len(raw), SPAN, points, plain[1:])


def check_window_edge(eng):
    """One call.  Every forged range lies behind sound ranges of another stream: a forged interval's slot is never
    the scratch's first, so a decoder that read before its slot would read inside the allocation and be seen by its
    status or its bytes."""
    streams, srcs, blobs, ranges, bad = [], [], [], [], {}
    for name, p, raw, plain in window_edge_cases():
        s = len(streams)
        streams += [raw, raw]
        srcs += [plain, plain[1:]]
        blobs += [honest_blob(raw), forged_past(raw)]
        ranges += [(s, 0, len(plain)), (s, p - 1, 2), (s, p, 5)]
        forged = [(s + 1, p - 1, 3), (s + 1, 0, len(plain))] + ([(s + 1, 0, 1)] if p > 1 else [])
        for r in forged:
            bad[len(ranges)] = -1
            ranges.append(r)
    check_read(eng, srcs, streams, blobs, ranges, bad)


# ---- a clean decode of the wrong length ----
@functools.lru_cache(maxsize=None)
def short_interval_case(k=20):
    """Every block of the stream a point but block k + 1, and point k's bit_off that of block k + 1: interval k parses
    cleanly from there to its stop bit and makes fewer bytes than it promises; interval k - 1 runs on through block k.
    (With block k + 1 a point as well the two bit_offs would be equal, which no decoder gets to see.)
    -> (stream, blob, k)"""
    data = family(-15)[3]
    blocks = sm.walk(data, sm.DF_DEFLATE)[1]
    d = sm.Blob(sm.index_at(data, sm.DF_DEFLATE, lambda j, b: j != k + 1)[0])
    assert d.points[k][0] == blocks[k][0] and d.points[k + 1][0] == blocks[k + 2][0]
    d.points[k][0] = blocks[k + 1][0]
    return data, d.pack(), k


def check_short_interval(eng):
    data, blob, k = short_interval_case()
    b = sm.Blob(blob)
    offs = [p[1] for p in b.points]
    ranges = [(0, offs[j] + 1, 20) for j in range(b.n_points - 1)] + [(0, offs[k - 1] - 1, 2), (0, offs[k + 1] - 1, 2)]
    bad = {k - 1: INVALID_BUFFER, k: INVALID_BUFFER, len(ranges) - 2: INVALID_BUFFER, len(ranges) - 1: INVALID_BUFFER}
    check_read(eng, [mix()], [data], [blob], ranges, bad)


# ---- a batch beyond the wide kernels' reach ----
@functools.lru_cache(maxsize=None)
def batch800():
    """800 streams of both detectable containers: 734 of 0 to 3000 source bytes (eight of none, some stored, some with
    a flush in the middle; one of them with a damaged trailer), 66 of 100 to 140 KB at the settings of FAMILY (one of
    them truncated) -> (streams, sources, the two bad ones)"""
    rng = random.Random(800)
    jobs = []
    for i in range(734):
        n = 0 if i < 8 else rng.randrange(1, 3001)
        o = rng.randrange(len(mix()) - 3000)
        jobs.append((mix()[o:o + n], rng.choice((0, 0, 1, 6, 6, 9)), 8, n // 2 if 8 <= i < 60 and n >= 200 else 0))
    for i in range(66):
        n = 100000 + 601 * i
        lv, mem = FAMILY[i % 4]
        jobs.append((mix()[1000 * i:1000 * i + n], lv, mem, 0))
    rng.shuffle(jobs)
    streams, srcs = [], []
    for i, (src, lv, mem, flush_every) in enumerate(jobs):
        streams.append(deflate(src, lv, 31 if i % 3 else 15, mem, flush_every))
        srcs.append(src)
    hurt = next(i for i, s in enumerate(srcs) if 0 < len(s) <= 3000 and i % 3)  # (gzip: its CRC-32)
    cut = next(i for i, s in enumerate(srcs) if len(s) >= 100000)
    bad = bytearray(streams[hurt])
    bad[-6] ^= 0x40
    streams[hurt] = bytes(bad)
    streams[cut] = streams[cut][:len(streams[cut]) * 2 // 3]
    return streams, srcs, (hurt, cut)


def check_batch800(eng, monkeypatch):
    """The index build's narrow recording kernels (batches above ZH_INFLATE_WIDE streams, 768 unless set: the
    library reads it once a process, so it is asserted here, not set)."""
    assert int(os.environ.get("ZH_INFLATE_WIDE", "768")) < 800
    streams, srcs, bad = batch800()
    blobs, sts, outs = build(eng, streams, sm.DF_DETECT, SPAN)
    _, want_sts = eng.uncompress_batch(streams, sm.DF_DETECT)
    assert sts == want_sts and sts.count(OK) == 798
    want = [None if i in bad else model(d, sm.DF_DETECT)[0] for i, d in enumerate(streams)]
    for i in range(800):
        if i in bad:
            assert sts[i] != OK and blobs[i] is None and outs[i] is None, i
        else:
            assert blobs[i] == want[i] and outs[i] == srcs[i], i
    ranges, badr = [], {}
    for s in range(800):
        if s in bad:
            badr[len(ranges)] = INVALID_BUFFER
            ranges.append((s, 0, 10))
            continue
        b = sm.Blob(want[s])
        ranges.append((s, b.points[1][1] - 1, 2) if b.n_points > 2 else (s, len(srcs[s]) // 3, 50))
    check_read(eng, srcs, streams, blobs, ranges, badr)
    monkeypatch.setenv("ZH_SEEK_FIRST_CAP", "2")
    again, sts2 = eng.seek_index_batch(streams, sm.DF_DETECT, SPAN)
    assert again == want and sts2 == sts


# ---- the sanitized program's cases ----
def dump(path):
    """Writes the cases of tests/seek_main.cpp: cases.txt "NAME STREAMS FORMAT SPAN" a line; NAME_<s>.bin the stream,
    .src its plaintext, .blob the model's blob (empty: no index, a status that is not ZH_OK), .rblob the blob the
    ranges are read with; NAME.ranges "STREAM OFF LEN STATUS" a line (-1: any status but ZH_OK and ZH_ERR_CHECKSUM).
    -> (cases, ranges)"""
    os.makedirs(path, exist_ok=True)
    cases, n_ranges = [], 0

    def put(name, fmt, span, streams, srcs, blobs, rblobs, ranges):
        nonlocal n_ranges
        for s in range(len(streams)):
            for ext, blob in ((".bin", streams[s]), (".src", srcs[s]), (".blob", blobs[s] or b""), (".rblob", rblobs[s])):
                with open(os.path.join(path, "%s_%d%s" % (name, s, ext)), "wb") as f:
                    f.write(blob)
        with open(os.path.join(path, name + ".ranges"), "w") as f:
            for s, off, n, st in ranges:
                f.write("%d %d %d %d\n" % (s, off & M64, n & M64, st))
        cases.append("%s %d %d %d" % (name, len(streams), fmt, span))
        n_ranges += len(ranges)

    # two containers told apart, the ranges of every kind
    streams = [family(31)[1], family(15)[3]]
    blobs = [model(d, sm.DF_DETECT)[0] for d in streams]
    ranges = [r + (OK,) for s in range(2) for r in stream_ranges(s, blobs[s], len(mix()))[1:]]
    put("family", sm.DF_DETECT, SPAN, streams, [mix()] * 2, blobs, blobs, ranges)
    # small streams, one with a damaged trailer, one truncated
    streams, srcs = (x[3:9] for x in batch33())
    streams = list(streams) + [batch33()[0][20]]
    srcs = list(srcs) + [batch33()[1][20]]
    blobs = [None if i in (2, 6) else model(d, sm.DF_DETECT)[0] for i, d in enumerate(streams)]
    ranges = [(s, 30000, 5000, INVALID_BUFFER if s in (2, 6) else OK) for s in range(7)]
    put("small", sm.DF_DETECT, SPAN, streams, srcs, blobs, [b or b"" for b in blobs], ranges)
    # crafted streams; the empty member; zeros
    cs = crafted()
    blobs = [model(raw, sm.DF_DEFLATE)[0] for raw, _ in cs]
    ranges = [(s, SPAN - 1, 300, OK) for s in range(len(cs))] + [(len(cs) - 1, SPAN, 258, OK)]
    put("crafted", sm.DF_DEFLATE, SPAN, [raw for raw, _ in cs], [p for _, p in cs], blobs, blobs, ranges)
    empty = deflate(b"", 6, 31, 8)
    blob = model(empty, sm.DF_GZIP, 1 << 20)[0]
    put("empty", sm.DF_GZIP, 0, [empty], [b""], [blob], [blob], [(0, 0, 10, OK)])
    z = zeros_stream()
    blob = model(z, sm.DF_ZLIB)[0]
    put("zeros", sm.DF_ZLIB, SPAN, [z], [bytes(1 << 20)], [blob], [blob], [(0, (1 << 20) - 70000, M64, OK)])
    # damage: static forms of the blob, a flipped byte, a moved point
    data = family(31)[3]
    blob = model(data, sm.DF_GZIP)[0]
    forms = [f for _, f in static_damage(blob, len(data))]
    b = sm.Blob(blob)
    moved = sm.Blob(blob)
    moved.points[4][0] += 1
    rblobs = forms + [blob, moved.pack()]
    n = len(rblobs)
    ranges = [(s, 40000 + s, 100, INVALID_BUFFER) for s in range(len(forms))] + [(len(forms), 40000, 100, OK)]
    ranges += [(n - 1, b.points[4][1] + 1, 20, -1), (n - 1, b.points[5][1] + 1, 20, OK)]
    # (format -1: these streams are read only)
    put("damage", -1, SPAN, [data] * n, [mix()] * n, [None] * n, rblobs, ranges)
    k, at, st = next(p for p in damage_plan(data, blob, 1) if p[2] != OK)
    flipped = bytearray(data)
    flipped[at] ^= 0xff
    rs, touching = neighbour_ranges(0, b, k)
    ranges = [r + ((CHECKSUM if st == CHECKSUM else -1) if j in touching else OK,) for j, r in enumerate(rs)]
    put("flipped", -1, SPAN, [bytes(flipped)], [mix()], [None], [blob], ranges)
    # points at every block start, empty intervals among them
    d, fmt, src = dense_streams(True)[1]
    blob = dense_point_sets(True)[0][1][1]
    put("dense", -1, SPAN, [d], [src], [None], [blob], [r + (OK,) for r in dense_ranges(0, blob)])
    # a match one byte past the window: the forged range first and alone, its slot the scratch's first
    name, p, raw, plain = next(c for c in window_edge_cases() if c[0] == "dynamic P=4097 j=1 len=258")
    put("past", -1, SPAN, [raw], [plain[1:]], [None], [forged_past(raw)], [(0, p - 1, 3, -1)])
    # a clean decode of the wrong length
    data, blob, k = short_interval_case()
    offs = [q[1] for q in sm.Blob(blob).points]
    ranges = [(0, offs[j] + 1, 20, INVALID_BUFFER if j in (k - 1, k) else OK) for j in range(k - 2, k + 2)]
    put("swap", -1, SPAN, [data], [mix()], [None], [blob], ranges)
    with open(os.path.join(path, "cases.txt"), "w") as f:
        f.write("\n".join(cases) + "\n")
    return len(cases), n_ranges
