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
    with open(os.path.join(path, "cases.txt"), "w") as f:
        f.write("\n".join(cases) + "\n")
    return len(cases), n_ranges
