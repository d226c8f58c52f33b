"""CPU-only, no engine: the model of the seek index (tests/seek_model.py) against Python's zlib -- its inflate on every
stream the seek cases use, its interval decode (from a point's bit, with the point's window, up to the next point's
bit) against the slice of the plaintext for every interval of every case, its blob against its own reader."""
import zlib

import seek_cases as sc
import seek_model as sm


def case_streams():
    """(stream, format) of every case"""
    out = [(d, fmt) for wbits, fmt in sc.WBITS for d in sc.family(wbits)]
    out += sc.flushed_streams() + [(sc.double_flush(), sm.DF_DEFLATE), (sc.zeros_stream(), sm.DF_ZLIB)]
    out += [(sc.deflate(b"", 6, 31, 8), sm.DF_GZIP)] + [(raw, sm.DF_DEFLATE) for raw, _ in sc.crafted()]
    streams, _ = sc.batch33()
    return out + [(d, sm.DF_DETECT) for i, d in enumerate(streams) if i not in (5, 20)]


WBITS_OF = {sm.DF_DEFLATE: -15, sm.DF_ZLIB: 15, sm.DF_GZIP: 31}


def test_model_inflate_equals_zlib_and_intervals_equal_slices():
    n_intervals = 0
    for data, fmt in case_streams():
        fmt = sm.resolve_format(data, fmt)
        blob, plain = sc.model(data, fmt)
        assert plain == zlib.decompress(data, WBITS_OF[fmt])
        b = sm.Blob(blob)
        assert b.pack() == blob and (b.magic, b.version, b.fmt, b.src_len, b.total) == (sm.MAGIC, 1, fmt, len(data), len(plain))
        assert b.points[0][1:4] == [0, 0, 0] and b.points[-1][1:] == [len(plain), b.window_bytes, 0, 0]
        for k in range(b.n_points - 1):
            p, q = b.points[k], b.points[k + 1]
            assert p[3] == min(p[1], sm.WINDOW) and p[2] % 16 == 0 and (k == 0 or q[1] - p[1] >= b.span or k + 2 == b.n_points)
            assert sm.decode_interval(data, b, k) == (sm.OK, plain[p[1]:q[1]]), k
            n_intervals += 1
    assert n_intervals > 150


def test_model_point_counts_of_the_first_family():
    for j, data in enumerate(sc.family(-15)):
        _, blocks, _ = sm.inflate(data, 0)
        assert (len(blocks), sm.Blob(sc.model(data, sm.DF_DEFLATE)[0]).n_points - 1) == ((3, 383, 628, 47)[j], sc.FAMILY_POINTS[j])
    assert sm.Blob(sc.model(sc.zeros_stream(), sm.DF_ZLIB)[0]).n_points - 1 >= 16


def test_model_sees_damage():
    """a flipped byte inside an interval: the model fails it or finds other bytes, as the plans of the damage cases say"""
    data = sc.family(-15)[1]
    blob = sc.model(data, sm.DF_DEFLATE)[0]
    plan = sc.damage_plan(data, blob, 1)
    assert len(plan) == 16 and sum(st == sm.OK for _, _, st in plan) <= 2
    assert {st for _, _, st in plan} <= {sm.OK, sm.INVALID_BUFFER, sm.CHECKSUM}


def test_model_upload_arithmetic():
    data = sc.family(31)[1]
    b = sm.Blob(sc.model(data, sm.DF_GZIP)[0])
    assert b.touched(b.total, 5) == [] and b.touched(5, 0) == [] and b.touched(0, 1 << 70) == list(range(b.n_points - 1))
    k = 4
    one = sm.upload_bytes([b], [len(data)], [(0, b.points[k][1] + 5, 10)])
    span = (b.points[k + 1][0] + 7) // 8 - b.points[k][0] // 8
    assert one == sm.pad16(span) + 32768
    assert sm.upload_bytes([b], [len(data)], [(0, b.points[k][1] + 5, 10)] * 3) == one


# ---- the premises of the cases with points at any block boundary: every blob is what its case says it is ----
def all_ok(data, blob):
    b = sm.Blob(blob)
    return all(sm.decode_interval(data, b, k)[0] == sm.OK for k in range(b.n_points - 1))


def test_model_index_at_and_sound():
    """index_at at the points the rule chooses is build_index's blob; sound() takes it and refuses every statically
    damaged form of the existing cases"""
    data = sc.family(31)[3]
    blob, plain = sc.model(data, sm.DF_GZIP)
    chosen = {tuple(p[:2]) for p in sm.Blob(blob).points}
    assert sm.index_at(data, sm.DF_GZIP, lambda j, b: b in chosen) == (blob, plain)
    assert sm.sound(blob, len(data))
    for name, form in sc.static_damage(blob, len(data)):
        assert not sm.sound(form, len(data)), name
    b = sm.Blob(sm.index_at(sc.double_flush(), sm.DF_DEFLATE, sc.every_block)[0])
    offs = [p[1] for p in b.points]
    # (6 blocks, 3 of them at an out_off another block has; the last block is empty too: 4 empty intervals)
    assert b.n_points == 7 and sum(offs[k] == offs[k + 1] for k in range(5)) == 3 and offs[5] == offs[6]
    assert b.touched(39999, 2) == [0, 1, 2, 3] and sm.decoded(b, 39999, 2) == [0, 3]
    assert [p[1] for p in sm.Blob(sm.index_at(sc.family(-15)[1], sm.DF_DEFLATE, sc.every_block)[0]).points[1:4]] == [8033, 17471, 26681]


def test_model_dense_point_sets():
    streams = sc.dense_streams()
    wins = set()
    for name, blobs in sc.dense_point_sets():
        for (data, fmt, src), blob in zip(streams, blobs):
            b = sm.Blob(blob)
            assert sm.sound(blob, len(data)) and b.total == len(src), name
            assert zlib.decompress(data, WBITS_OF[fmt]) == src
            for k in range(b.n_points - 1):
                assert sm.decode_interval(data, b, k) == (sm.OK, src[b.points[k][1]:b.points[k + 1][1]]), (name, k)
            wins |= {p[3] for p in b.points[:-1]}
            if name == "the youngest":
                assert b.n_points <= 3 and all(p[3] < sm.WINDOW for p in b.points)
        if name == "every block":
            assert [sm.Blob(b).n_points - 1 for b in blobs[:4]] == [383, 6, 628, 47]
    between = {w for w in wins if 0 < w < sm.WINDOW}
    assert {0, sm.WINDOW} <= wins and len(between) >= 3 and any(w % 16 for w in between)
    # the emulator's subset is the first two streams of these
    assert [d for d, _, _ in sc.dense_streams(True)] == [d for d, _, _ in streams[:2]]


def test_model_crafted_behind_history():
    for small in (True, False):
        cases = sc.parity_crafted(small)
        good = [c for c in cases if c[2] is not None]
        assert len(good) == (45 if small else 90) and len(cases) == (104 if small else 158)
        for name, raw, plain, _ in good:
            assert sc.model(raw, sm.DF_DEFLATE)[1] == plain, name
        behind = sc.behind_history(small)
        assert {h for _, h, _, _ in behind} == ({4097} if small else set(sc.HISTORIES))
        empties = 0
        for name, h, data, plain in behind:
            blob, got = sm.index_at(data, sm.DF_DEFLATE, sc.every_block)
            b = sm.Blob(blob)
            assert got == plain and sm.sound(blob, len(data)), name  # (the builder's plaintext: zlib refuses some of these)
            assert b.points[1][1] == h and b.points[1][3] == min(h, sm.WINDOW) and all_ok(data, blob), name
            empties += sum(b.points[k][1] == b.points[k + 1][1] for k in range(b.n_points - 1))
        assert empties > (100 if small else 10000)


def test_model_window_edge():
    """a match at the window's first byte: [OK, OK]; the forged blob passes every static rule and both its intervals
    fail, the second one by its match's distance"""
    ps = set()
    for name, p, raw, plain in sc.window_edge_cases():
        assert zlib.decompress(raw, -15) == plain, name
        honest, forged = sc.honest_blob(raw), sc.forged_past(raw)
        assert sm.sound(honest, len(raw)) and sm.sound(forged, len(raw)), name
        b, f = sm.Blob(honest), sm.Blob(forged)
        assert [sm.decode_interval(raw, b, k)[0] for k in (0, 1)] == [sm.OK, sm.OK], name
        assert [sm.decode_interval(raw, f, k)[0] for k in (0, 1)] == [sm.INVALID_BUFFER, sm.INVALID_BUFFER], name
        assert b.points[1][3] == min(p, sm.WINDOW) and f.points[1][3] == min(p, sm.WINDOW) - 1
        # (one byte more of history and the forged interval decodes: it is the distance that fails it)
        q = f.points[1]
        assert sm.inflate(raw, q[0], plain[:p], stop=f.points[2][0])[0] == plain[p:], name
        ps |= {b.points[1][3], f.points[1][3]}
    assert ps == {0, 1, 2, 257, 258, 4096, 4097, 32766, 32767, 32768}


def test_model_short_interval():
    data, blob, k = sc.short_interval_case()
    b = sm.Blob(blob)
    assert sm.sound(blob, len(data)) and b.n_points - 1 == 46
    for j in range(b.n_points - 1):
        want = sm.INVALID_BUFFER if j in (k - 1, k) else sm.OK
        assert sm.decode_interval(data, b, j)[0] == want, j
    # interval k parses cleanly up to its stop bit and is short: what fails it is the count of its bytes alone
    p, q = b.points[k], b.points[k + 1]
    got, _, end = sm.inflate(data, p[0], b.window(k), stop=q[0], limit=q[1] - p[1])
    assert end == q[0] and 0 < len(got) < q[1] - p[1]


def test_model_batch_of_800():
    streams, srcs, bad = sc.batch800()
    assert len(streams) == 800 and len(set(bad)) == 2
    assert sum(len(s) <= 3000 for s in srcs) == 734 and sum(len(s) == 0 for s in srcs) == 8
    assert sum(100000 <= len(s) <= 140000 for s in srcs) == 66
    one, several, three_points = 0, 0, 0
    for i, data in enumerate(streams):
        if i in bad:
            continue
        fmt = sm.resolve_format(data, sm.DF_DETECT)
        blob, plain = sc.model(data, sm.DF_DETECT)
        assert plain == srcs[i] == zlib.decompress(data, WBITS_OF[fmt])
        blocks = sm.walk(data, fmt)[1]
        one += len(blocks) == 1
        several += len(blocks) > 1
        three_points += sm.Blob(blob).n_points - 1 >= 3
    assert one >= 600 and several >= 64 and three_points >= 32, (one, several, three_points)
    for i in bad:
        try:
            zlib.decompress(streams[i], 47)
            raise AssertionError("stream %d is sound" % i)
        except zlib.error:
            pass
    assert sum(d[:2] == b"\x1f\x8b" for d in streams) > 400 and sum(d[:1] == b"\x78" for d in streams) > 200
    assert any(sm.walk(d, sm.resolve_format(d, 0))[1] and d[sm.body_bit(d, sm.resolve_format(d, 0)) // 8] & 6 == 0
               for i, d in enumerate(streams) if i not in bad and len(srcs[i]) <= 3000)  # (stored blocks)
