"""Shared by tests/test_emu_zip_read_batch.py and tests/test_gpu_zip_read_batch.py: zip images made record by record
(struct + zlib raw deflate), and the check of zh_zip_read_batch (Engine.read_zips) against tests/zip_v1_reader_model.py
(ziparchives_v1.nim's openStreamImpl restated).  Where the model's decoder rejects a stream, the status to equal is the
one Engine.uncompress_batch gives the same bytes (the oracle's codes for a damaged stream are the codec's own).

The scan's geometry (zh_zip_read_batch.hip): a lane reads 16 bytes, a wave 1024, a workgroup 4096 a step and 16384 in
all; the walk's scan covers 1024 nodes a workgroup."""
import os
import random
import struct
import zlib

import zip_v1_reader_model as zm
from zippy_amd.common import ZippyError

OK, ARCHIVE_EOF, ARGUMENT, METHOD, CRC = 0, 23, 22, 25, 27
DATA_DESCRIPTOR, DEFLATE64, SIZE, OPEN = 42, 43, 44, 45
DECODER = "decoder"  # a status of the codec: whatever Engine.uncompress_batch says of the stream
LOCAL_SIG, CENTRAL_SIG, END_SIG = 0x04034B50, 0x02014B50, 0x06054B50
SCAN_CHUNKS = (16, 1024, 4096, 16384)  # bytes a lane, a wave, a workgroup's step, a workgroup of the scan cover
WALK_GROUP = 1024
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ziparchives")
T0, D0 = 0x6000, 0x5521


def blob(n, seed=1):
    """n bytes without a 'P'"""
    return bytes(((i * 131 + seed * 7 + (i >> 5) * 3) & 0xFF) or 1 for i in range(n)).replace(b"P", b"Q")


def deflate(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def L(name, data=b"", method=8, **kw):
    """a local record.  Overrides: flags, extra, stream (the bytes in the image), crc, usize, csize, time, date"""
    return dict(kw, kind="L", name=name, data=data, method=method)


def C(name, external=0x20, **kw):
    """a central record.  Overrides: extra, comment"""
    return dict(kw, kind="C", name=name, external=external)


def END(comment=b"", **kw):
    return dict(kw, kind="E", comment=comment)


def record(r):
    if r["kind"] == "L":
        data = r["data"]
        stream = r.get("stream", deflate(data) if r["method"] == 8 else data)
        extra = r.get("extra", b"")
        return struct.pack("<IHHHHHIIIHH", LOCAL_SIG, 20, r.get("flags", 0x0800), r["method"], r.get("time", T0),
                           r.get("date", D0), r.get("crc", zlib.crc32(data)), r.get("csize", len(stream)),
                           r.get("usize", len(data)), len(r["name"]), len(extra)) + r["name"] + extra + stream
    if r["kind"] == "C":
        extra, comment = r.get("extra", b""), r.get("comment", b"")
        return struct.pack("<IHHHHHHIIIHHHHHII", CENTRAL_SIG, 63, 20, 0x0800, 0, T0, D0, 0, 0, 0, len(r["name"]),
                           len(extra), len(comment), 0, 0, r["external"], 0) + r["name"] + extra + comment
    comment = r["comment"]
    return struct.pack("<IHHHHIIH", END_SIG, 0, 0, 0, 0, 0, 0, r.get("clen", len(comment))) + comment


def build(records):
    return b"".join(record(r) for r in records)


def archive(entries, central=True, end=True, tail=b""):
    """the local records, a central record for each (its raw name), the end record"""
    rs = list(entries)
    if central:
        rs += [C(e["name"], 0x10 if e["name"].endswith(b"/") else 0x20) for e in entries]
    if end:
        rs.append(END())
    return build(rs) + tail


def good_images():
    a = archive([L(b"dir/", b"", 0), L(b"dir/a.txt", b"alpha" * 40), L(b"dir/b.bin", blob(3000)), L(b"empty", b"", 0)])
    b = archive([L(b"s/one", blob(700, 2), 0), L(b"s/two", blob(5000, 3))], central=False)
    return [a, b]


def fixture(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def fake_archive():
    return archive([L(b"decoy.txt", b"never reached", 0), L(b"decoy2", blob(40, 9))])


# ---- the cases: lists of (id, image, status); None: whatever the model says ----
def _end_at(p):
    """an archive whose end record starts at image position p >= 31, behind one stored entry"""
    return build([L(b"a", b"\x41" * (p - 31), 0), END()])


def scan_geometry():
    out = [("end_at_mod16_%d" % (p % 16), _end_at(p), OK) for p in range(64, 80)]
    for c in SCAN_CHUNKS:
        for k in (1, 2):
            for d in range(-3, 4):
                out.append(("end_at_%dx%d%+d" % (k, c, d), _end_at(k * c + d), OK))
    a = build([L(b"a", b"x", 0)])
    out.append(("signature_in_last_4_bytes", a + b"PK\5\6", ARCHIVE_EOF))
    out.append(("local_in_last_4_bytes", a + b"PK\3\4", ARCHIVE_EOF))
    end = build([END()])
    out += [("len0", b"", ARCHIVE_EOF), ("len1", end[:1], ARCHIVE_EOF), ("len3", end[:3], ARCHIVE_EOF),
            ("len4", end[:4], ARCHIVE_EOF), ("len4_no_signature", b"PK\7\x08", OPEN), ("len21", end[:21], ARCHIVE_EOF),
            ("len22", end, OK), ("len23", end + b"\0", OK), ("no_signature_at_all", b"\x41" * 5000, OPEN)]
    return out


def straddling_pair():
    """two images whose tail plus head spell a signature: no padding lies between them (a length that is a multiple
    of 8), and the first one's walk steps onto its last two bytes"""
    a = build([L(b"abcd", b"\x41" * 12, 0)]) + b"PK"  # 48
    assert len(a) % 8 == 0
    return [("tail_PK", a, ARCHIVE_EOF), ("head_0506", b"\5\6" + build([END()])[4:] + b"\0\0", OPEN)]


CHAIN_LENGTHS = sorted(set([0, 1, 2, 3] + [n for k in range(2, 12) for n in ((1 << k) - 1, 1 << k, (1 << k) + 1)]))


def chain(n, central, tag=b"e"):
    """n empty stored entries with short names: n + 1 hits without a central directory, 2n + 1 with one"""
    return archive([L(tag + b"%d" % i, b"", 0) for i in range(n)], central=central)


# hits (and, with the image's END node, nodes) of 1022 .. 1026 and 2046 .. 2050 around the walk's scan group of 1024
HIT_COUNT_LENGTHS = [1021, 1022, 2045, 2046]


def chains():
    return [("chain%d%s" % (n, "c" if c else ""), chain(n, c), OK) for n in CHAIN_LENGTHS for c in (False, True)] + [
        ("chain%d" % n, chain(n, False), OK) for n in HIT_COUNT_LENGTHS]


def decoys():
    d = fake_archive()
    es = [L(b"a", b"A"), L(b"b", b"B", 0)]
    body = b"head" + d + b"tail"
    stored_block = deflate(body, 0)  # a stored deflate block: the fake archive's bytes lie open in the stream
    assert b"PK\3\4" in stored_block
    return [("in_stored_entry", archive([es[0], L(b"data.bin", body, 0), es[1]]), OK),
            ("in_extra_field", archive([es[0], L(b"x", b"X", extra=struct.pack("<HH", 0x9999, len(d)) + d), es[1]]), OK),
            ("in_name", archive([es[0], L(b"n" + d, b"N"), es[1]]), OK),
            ("in_central_comment", build(es + [C(b"a", comment=d), C(b"b", extra=d), END()]), OK),
            ("behind_end_record", archive(es, tail=d), OK),
            ("in_end_comment", build(es + [END(comment=d)]), OK),
            ("in_deflate_stream", archive([es[0], L(b"s", body, 8, stream=stored_block), es[1]]), OK)]


def statuses():
    data = blob(2000, 11)
    st = deflate(data)
    broken = b"\x07" + st[1:]  # a final block of the reserved type 3
    pre, post = L(b"pre", blob(100, 1), 0), L(b"post", blob(1500, 2))
    ok = archive([pre, post])

    def one(**kw):
        return archive([pre, L(b"x", data, **kw), post])

    def one0(**kw):
        return archive([pre, L(b"x", data, 0, **kw), post])
    cut_in_name = build([pre, L(b"x" * 40, data)])
    cen = build([pre, C(b"pre", extra=b"ee" * 10, comment=b"cc" * 10)])
    return [
        ("data_descriptor", one(flags=4), DATA_DESCRIPTOR), ("deflate64", one(flags=8), DEFLATE64),
        ("method", one(method=9, stream=st), METHOD),
        ("dd_before_d64", one(flags=12), DATA_DESCRIPTOR),
        ("d64_before_method", one(flags=8, method=9, stream=st), DEFLATE64),
        ("dd_before_eof", build([pre, L(b"x" * 40, data, flags=4)])[:180], DATA_DESCRIPTOR),
        ("method_before_eof", build([pre, L(b"x" * 40, data, method=9, stream=st)])[:180], METHOD),
        ("local_header_cut", build([pre, L(b"x", data)])[:len(build([pre])) + 29], ARCHIVE_EOF),
        ("local_header_whole_no_name", build([pre, L(b"x", data)])[:len(build([pre])) + 30], ARCHIVE_EOF),
        ("name_beyond", cut_in_name[:len(build([pre])) + 50], ARCHIVE_EOF),
        ("data_beyond", build([pre, L(b"x", data)])[:-1], ARCHIVE_EOF),
        ("csize_ffffffff", one0(csize=0xFFFFFFFF), ARCHIVE_EOF),
        ("central_cut", cen[:len(build([pre])) + 45], ARCHIVE_EOF),
        ("central_comment_beyond", cen[:-1], ARCHIVE_EOF),
        ("central_whole_no_end", cen, ARCHIVE_EOF),
        ("end_cut", ok[:-1], ARCHIVE_EOF), ("end_comment_beyond", build([pre, END(b"abc", clen=4)]), ARCHIVE_EOF),
        ("no_end_record", archive([pre, post], end=False), ARCHIVE_EOF),
        ("no_end_record_no_directory", archive([pre, post], central=False, end=False), ARCHIVE_EOF),
        ("starts_with_central", build([C(b"pre"), pre, END()]), OPEN),
        ("junk_in_front", b"junk" + ok, OPEN),
        ("target_in_last_3_bytes", build([pre]) + b"PK\5", ARCHIVE_EOF),
        ("target_on_non_signature", build([pre]) + b"junk" * 2, OPEN),
        ("target_on_other_signature", build([pre]) + b"PK\7\x08" + b"\0" * 30, OPEN),
        ("crc_stored", one0(crc=5), CRC), ("crc_deflated", one(crc=zlib.crc32(data) ^ 1), CRC),
        ("damaged_stream", one(stream=broken), DECODER), ("cut_stream", one(stream=st[:len(st) // 2]), DECODER),
        ("decoder_before_crc", one(stream=broken, crc=1), DECODER),
        ("crc_before_size", one(crc=1, usize=5), CRC), ("crc_before_size_stored", one0(crc=1, usize=5), CRC),
        ("crc_before_size_overstated", one(crc=1, usize=len(data) + 9), CRC),
        ("usize_overstated", one(usize=len(data) + 5000), SIZE), ("usize_understated", one(usize=100), SIZE),
        ("usize_understated_0", one(usize=0), SIZE), ("usize_understated_by_1", one(usize=len(data) - 1), SIZE),
        ("usize_overstated_stored", one0(usize=len(data) + 1), SIZE), ("usize_understated_stored", one0(usize=3), SIZE),
        ("usize_ffffffff_tiny_image", archive([L(b"t", b"tiny", usize=0xFFFFFFFF)]), SIZE),
        ("usize_ffffffff_stored", archive([L(b"t", b"tiny", 0, usize=0xFFFFFFFF)]), SIZE),
        ("deflated_csize_0", archive([pre, L(b"z", b"", 8, stream=b""), post]), DECODER),
        ("empty_deflated", archive([pre, L(b"z", b"", 8), post]), OK), ("empty_stored", archive([pre, L(b"z", b"", 0), post]), OK),
        ("bad_in_the_middle", archive([pre, L(b"x", data, crc=3), L(b"y", data, flags=4), L(b"z", data, method=77)]), CRC),
        ("header_failure_behind_bad_crc", build([pre, L(b"x", data, crc=3), C(b"nobody"), END()]), CRC),
        ("bad_crc_behind_missing_key", build([pre, C(b"nobody"), L(b"x", data, crc=3), END()]), OPEN),
        ("broken_behind_end_record", archive([pre, post], tail=build([L(b"x", data, crc=3, flags=12)])[:50]), OK),
        ("junk_behind_end_record", archive([pre, post], tail=b"junk" * 9), OK)]


def tables():
    a1, a2 = L(b"a", b"first", 0, time=1, date=2), L(b"a", b"second, and longer", time=3, date=4)
    b, c = L(b"b", blob(300, 5)), L(b"c", b"C", 0)
    return [("duplicate_key", archive([a1, b, a2, c], central=False), OK),
            ("duplicate_key_with_directory", build([a1, b, a2, c, C(b"a", 0o100644 << 16), C(b"b"), END()]), OK),
            ("backslash_and_slash", build([L(b"a\\b", b"1", 0), c, L(b"a/b", b"2"), C(b"a/b"), END()]), OK),
            ("backslash_key_found_by_slash", build([L(b"d\\e\\f", b"1", 0), C(b"d/e/f", 0x10), END()]), OK),
            ("backslash_in_directory", build([L(b"a\\b", b"1", 0), C(b"a\\b"), END()]), OPEN),
            ("central_before_its_entry", build([c, C(b"b"), b, END()]), OPEN),
            ("two_centrals", build([b, c, C(b"b", 0x10 | (0o040755 << 16)), C(b"b", 0o100600 << 16), C(b"c", 0x10), END()]), OK),
            ("no_central_records", archive([b, c], central=False), OK),
            ("some_central_records", build([b, c, C(b"c", 0o100755 << 16), END()]), OK),
            ("directory_with_bytes", build([L(b"d/", b"kept", 0), C(b"d/", 0x10), END()]), OK),
            ("empty_name", build([L(b"", b"nameless"), C(b""), END()]), OK),
            ("long_names", archive([L(b"n" * 65535, b"N"), L(b"m\\" * 300, b"M", 0)], central=False), OK),
            ("no_entries", build([END()]), OK)]


ALIGN_LEN = 4097


def alignment():
    """one archive of stored entries of 4097 bytes (several 16-byte chunks and both edges) whose data start at every
    address mod 16, twice over: consecutive slots of the output lie 8 mod 16 apart"""
    es, at = [], 0
    for i in range(32):
        name = b"r%02d" % i
        start = at + 30 + len(name) + 4
        pad = (i % 16 - start) % 16
        es.append(L(name, blob(ALIGN_LEN, 20 + i), 0, extra=struct.pack("<HH", 0x4141, pad) + b"." * pad))
        at = start + pad + ALIGN_LEN
    return archive(es)


def copy_shifts(image, reader):
    """the distances mod 16 between where the entries lie in the image and in the reader's block"""
    block, out = reader.data, set()
    for i in range(len(reader.entries)):
        data = reader.contents(i)
        assert image.count(data) == 1 and block.count(data) == 1
        out.add((image.index(data) - block.index(data)) % 16)
    return out


_MUTATIONS = ["none"] * 9 + ["crc", "flags4", "flags8", "method", "cut", "stream", "usize", "no_end", "junk", "missing_key",
                             "prefix", "dup", "backslash"]


def random_images(seed, n):
    """n small archives from a seeded generator, more than half of them intact"""
    rng = random.Random(seed)
    out = []
    for t in range(n):
        es = []
        for i in range(rng.randrange(0, 9)):
            k = rng.choice([0, 1, 17, 300, 2500])
            name = b"t%d/%s%d" % (t, rng.choice([b"f", b"g" * 40, b"caf\x82"]), i)
            es.append(L(name, blob(k, t + i), rng.choice([0, 8, 8]), time=rng.randrange(65536), date=rng.randrange(65536)))
        m = rng.choice(_MUTATIONS)
        if not es and m not in ("cut", "no_end", "junk", "prefix", "missing_key"):
            m = "none"
        e = rng.choice(es) if es else None
        cs = [C(x["name"], rng.choice([0x20, 0x10, 0o100644 << 16])) for x in es if rng.random() < 0.8]
        end = [END(b"c" * rng.randrange(0, 5))]
        if m == "crc":
            e["crc"] = 7
        elif m == "flags4":
            e["flags"] = 4
        elif m == "flags8":
            e["flags"] = 0x808
        elif m == "method":
            e["stream"] = deflate(e["data"]) if e["method"] == 8 else e["data"]
            e["method"] = 12
        elif m == "stream" and e["method"] == 8 and len(e["data"]) > 100:
            e["stream"] = b"\x07" + deflate(e["data"])[1:]
        elif m == "usize":
            e["usize"] = rng.choice([0, 3, len(e["data"]) + 100])
        elif m == "no_end":
            end = []
        elif m == "missing_key":
            cs.insert(rng.randrange(len(cs) + 1), C(b"nobody"))
        elif m == "dup":
            es.append(dict(e, data=blob(33, t)))
        elif m == "backslash":
            e["name"] = e["name"].replace(b"/", b"\\")
        img = build(es + cs + end)
        if m == "cut":
            img = img[:rng.randrange(0, len(img))]
        elif m == "junk":
            img += b"\x7f" * rng.randrange(1, 50)
        elif m == "prefix":
            img = b"\x7f" * rng.randrange(1, 50) + img
        out.append(img)
    return out


# ---- the check ----
_decoder = {}


def decoder_status(eng, stream):
    if stream not in _decoder:
        _decoder[stream] = eng.uncompress_batch([stream], 3)[1][0]
        assert _decoder[stream] not in (OK, ARCHIVE_EOF, METHOD, CRC, DATA_DESCRIPTOR, DEFLATE64, SIZE, OPEN)
    return _decoder[stream]


def check_batch(eng, images, want=None, close_order=None):
    """Open `images` in ONE call and hold every status, the key order, every field, every entry_v1 triple and every
    byte against the model (and against `want`, the statuses the cases were built for).  -> the statuses"""
    images = [bytes(b) for b in images]
    readers, sts = eng.read_zips(images)
    try:
        assert len(readers) == len(sts) == len(images)
        for t, image in enumerate(images):
            st, table, stop = zm.expected(image)
            tag = "image %d" % t
            if want is not None and want[t] is not None:
                assert (DECODER if st is None else st) == want[t], "%s: the model says %r, built for %r" % (tag, st, want[t])
            if table is None:
                if st is None:
                    st = decoder_status(eng, stop.stream)
                assert sts[t] == st, "%s: status %d, the model says %d" % (tag, sts[t], st)
                assert readers[t] is None, tag
                continue
            r = readers[t]
            assert sts[t] == OK and r is not None, "%s: status %d, the model opens it" % (tag, sts[t])
            assert [e["path"] for e in r.entries] == [k.decode("utf-8", "surrogateescape") for k in table], tag
            block = r.data
            assert len(block) % 8 == 0
            for i, (key, v) in enumerate(table.items()):
                where = "%s entry %d (%r)" % (tag, i, key[:40])
                e = r.entries[i]
                for f in ("is_directory", "unix_mode", "header_offset", "compressed_size", "uncompressed_size", "crc32"):
                    assert e[f] == v[f], "%s: %s" % (where, f)
                assert r.entry_v1(i) == (v["dos_time"], v["dos_date"], v["in_directory"]), where
                assert r.entry_status(i) == OK and r.contents(i) == v["contents"], where
                assert r.find(e["path"]) == i, where
                if v["contents"]:
                    assert v["contents"] in block, where
            with_error(ARGUMENT, lambda: r.extract_batch([0] if table else []))
            with_error(ARGUMENT, lambda: r.entry_v1(len(table)))
    finally:
        order = list(range(len(readers))) if close_order is None else close_order
        for t in order:
            if readers[t] is not None:
                readers[t].close()
    return sts


def with_error(status, fn):
    try:
        fn()
    except ZippyError as e:
        assert e.status == status, e.status
    else:
        raise AssertionError("no error %d" % status)


def alone_between_neighbours(eng, image, status):
    good = good_images()
    sts = check_batch(eng, [good[0], image, good[1]], want=[OK, status, OK])
    assert sts[0] == sts[2] == OK
    return sts[1]


def dump(directory, cases):
    """cases as files (for the stand-alone sanitizer driver): NAME.zip + expected.txt; a decoder status is written
    as -1 (any status outside the archive layer's)"""
    os.makedirs(directory, exist_ok=True)
    lines = []
    for name, image, _ in cases:
        with open(os.path.join(directory, name + ".zip"), "wb") as f:
            f.write(image)
        st = zm.expected(image)[0]
        lines.append("%s.zip %d" % (name, -1 if st is None else st))
    with open(os.path.join(directory, "expected.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(lines)
