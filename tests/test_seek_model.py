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
