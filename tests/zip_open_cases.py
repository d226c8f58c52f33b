"""Shared by tests/test_emu_zip_open_batch.py and tests/test_gpu_zip_open_batch.py: zip images made by hand (struct +
zlib raw deflate) and by zipfile, and the check of zh_zip_open_all_batch (Engine.open_zips) against its two referees --
oracle/zip_oracle.py's open_archive / extract_file (ziparchives.nim restated) plus internal.nim's path rule, and
Engine.open_zip / extract_batch on every image by itself."""
import io
import os
import random
import struct
import zipfile
import zlib

from oracle import ZippyError as OracleError
from oracle import zip_oracle
from zippy_amd.common import ZippyError

ARCHIVE_EOF, FILE_HEADER, METHOD, NO_RECORD, CRC, UNSUPPORTED, CENTRAL_HEADER = 23, 24, 25, 26, 27, 28, 29
DISK_NUMBER, DUPLICATE, CENTRAL_SIZE, UNSAFE_PATH, ARGUMENT = 30, 31, 32, 35, 22

_MESSAGES = {"Unexpected EOF": ARCHIVE_EOF, "Unsupported archive, disk number": UNSUPPORTED,
             "Unsupported archive, num disks": UNSUPPORTED, "Unsupported archive, start disk": UNSUPPORTED,
             "Unsupported archive, record number": UNSUPPORTED, "Invalid central directory file header": CENTRAL_HEADER,
             "Unsupported archive, compression method": METHOD, "Invalid file disk number": DISK_NUMBER,
             "Unsupported archive, duplicate entry": DUPLICATE, "Invalid central directory size": CENTRAL_SIZE,
             "Invalid file header": FILE_HEADER, "Verifying crc32 failed": CRC, "No file record": NO_RECORD}

FILE_SIG, CENTRAL_SIG, EOCD_SIG, Z64_EOCD_SIG, Z64_LOC_SIG = 0x04034B50, 0x02014B50, 0x06054B50, 0x06064B50, 0x07064B50
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ziparchives")


def blob(n, seed=1):
    return bytes((i * 131 + seed * 7 + (i >> 5) * 3) & 0xFF for i in range(n))


def deflate(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def E(name, data=b"", method=8, **kw):
    """One entry.  Overrides: flags, lextra, cextra, comment, external, stream (the bytes stored in the archive),
    crc, c_method, l_method, l_sig, c_sig, c_csize, c_usize, c_hoff, disk."""
    d = dict(name=name, data=data, method=method)
    d.update(kw)
    return d


def central(e, hoff, stream, crc):
    name, cextra, comment = e["name"], e.get("cextra", b""), e.get("comment", b"")
    return struct.pack("<IHHHHHHIIIHHHHHII", e.get("c_sig", CENTRAL_SIG), 20, 20, e.get("flags", 0x0800),
                       e.get("c_method", e["method"]), 0, 0, crc, e.get("c_csize", len(stream)),
                       e.get("c_usize", len(e["data"])), len(name), len(cextra), len(comment), e.get("disk", 0), 0,
                       e.get("external", 0), e.get("c_hoff", hoff)) + name + cextra + comment


def build(entries, prefix=b"", comment=b"", num=None, on_disk=None, cd_size_delta=0, disk=0, start_disk=0,
          zip64=None, cut=0, after_cd=b""):
    """A zip image.  prefix: junk in front (offsets do not count it).  zip64: None, or a dict of overrides for the
    zip64 end record and locator (loc_disk, disks, sig).  cut: bytes taken off the end of the central directory's last
    record, in an image whose directory lies behind its end record."""
    out = bytearray()
    cds = []
    for e in entries:
        data = e["data"]
        stream = e.get("stream", deflate(data) if e["method"] == 8 else data)
        crc = e.get("crc", zlib.crc32(data))
        name, lextra = e["name"], e.get("lextra", b"")
        hoff = len(out)
        out += struct.pack("<IHHHHHIIIHH", e.get("l_sig", FILE_SIG), 20, e.get("flags", 0x0800),
                           e.get("l_method", e["method"]), 0, 0, crc, len(stream) & 0xFFFFFFFF, len(data), len(name),
                           len(lextra)) + name + lextra + stream
        cds.append(central(e, hoff, stream, crc))
    if cut:  # the end record in FRONT of the directory, whose last record the image's end cuts
        cd = b"".join(cds)
        out += struct.pack("<IHHHHIIH", EOCD_SIG, 0, 0, len(entries), len(entries), len(cd), len(out) + 22, 0)
        return prefix + bytes(out) + cd[:-cut]
    cd_start = len(out)
    out += b"".join(cds) + after_cd
    cd_size = len(out) - cd_start + cd_size_delta
    n = len(entries) if num is None else num
    n_disk = n if on_disk is None else on_disk
    if zip64 is not None:
        z_at = len(out)
        out += struct.pack("<IQHHIIQQQQ", zip64.get("sig", Z64_EOCD_SIG), 44, 45, 45, disk, start_disk, n_disk, n, cd_size,
                           cd_start)
        out += struct.pack("<IIQI", Z64_LOC_SIG, zip64.get("loc_disk", 0), z_at + len(prefix), zip64.get("disks", 1))
        out += struct.pack("<IHHHHIIH", EOCD_SIG, 0, 0, 0xFFFF, 0xFFFF, 0xFFFFFFFF, 0xFFFFFFFF, len(comment))
    else:
        out += struct.pack("<IHHHHIIH", EOCD_SIG, disk, start_disk, n_disk, n, cd_size, cd_start, len(comment))
    return prefix + bytes(out) + comment


def chain(n, tag=b"e"):
    """n empty stored entries with short names"""
    return build([E(tag + b"%d" % i, b"", 0) for i in range(n)])


def zipfile_image(members, compression=zipfile.ZIP_DEFLATED):
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", compression) as zf:
        for name, data in members:
            zf.writestr(zipfile.ZipInfo(name, (2020, 1, 2, 3, 4, 6)), data, compression)
    return buf.getvalue()


def good_images():
    a = zipfile_image([("dir/", b""), ("dir/a.txt", b"alpha" * 40), ("dir/b.bin", blob(3000)), ("empty", b"")])
    b = build([E(b"s/one", blob(700, 2), 0), E(b"s/two", blob(5000, 3)), E(b"s/dir/", external=0x10, method=0)])
    c = zip_oracle.create_archive([("k/x.txt", b"x" * 999), ("k/y.txt", blob(2500, 5)), ("k/z", b"")])
    return [a, b, c]


def bagnon():
    with open(os.path.join(GOLDEN, "Bagnon-10.2.31.zip"), "rb") as f:
        return f.read()


# ---- the cases of the issue, as lists of (id, image) or (id, image, archive status) ----
def doubling_chains():
    ns = [1, 2, 3] + [n for k in range(2, 12) for n in ((1 << k) - 1, 1 << k, (1 << k) + 1)]
    return [("chain%d" % n, chain(n)) for n in sorted(set(ns))]


GEOMETRY_LENS = [0, 1, 63, 64, 65, 255, 65535]


def geometry():
    out = []
    mid = E(b"mid", blob(300, 4))
    for n in GEOMETRY_LENS:
        name = (b"n" * n)
        out.append(("name%d" % n, build([E(b"first", b"1", 0), E(name, blob(90, n), 8), mid])))
        if n >= 4:  # an extra field needs its 4-byte header
            ex = struct.pack("<HH", 0x7075, n - 4) + b"x" * (n - 4)
            out.append(("extra%d" % n, build([E(b"first", b"1", 0), E(b"ex", blob(90, n), 8, cextra=ex), mid])))
        else:
            out.append(("extra%d" % n, build([E(b"first", b"1", 0), E(b"ex", blob(90, n), 8, cextra=b"\x09" * n), mid]),
                        None))
        out.append(("comment%d" % n, build([E(b"first", b"1", 0), E(b"co", blob(90, n), 8, comment=b"c" * n), mid])))
    # an end record that overstates the directory's size (the nodes end where the chain can reach), and records of
    # the greatest length there is, which start exactly where that reach ends
    out.append(("cd_size_overstated", build([E(b"big", blob(6000, 3), 0), E(b"b", b"B")], cd_size_delta=5000)))
    full = dict(cextra=struct.pack("<HH", 0x7075, 65531) + b"x" * 65531, comment=b"c" * 65535)
    out.append(("longest_records", build([E(b"p" * 65535, b"1", 0, **full), E(b"q" * 65535, b"2", 0, **full),
                                          E(b"last", b"3", 0)])))
    out.append(("ends_at_cd_end", build([E(b"a", b"A"), E(b"b", b"B", comment=b"zz")])))
    out.append(("one_past_cd_end", build([E(b"a", b"A"), E(b"b", b"B", comment=b"zz")], cd_size_delta=-1), CENTRAL_SIZE))
    # (a comment or extra field cut by the image's end goes unnoticed by the reference: only the 46 bytes and the name count)
    out.append(("comment_cut_by_image_end", build([E(b"a", b"A"), E(b"b", b"B", comment=b"zz" * 30)], cut=10), 0))
    out.append(("name_cut_by_image_end", build([E(b"a", b"A"), E(b"b", b"B", comment=b"zz" * 30)], cut=61), ARCHIVE_EOF))
    out.append(("header_cut_by_image_end", build([E(b"a", b"A"), E(b"b", b"B", comment=b"zz" * 30)], cut=70), ARCHIVE_EOF))
    return [x if len(x) == 3 else x + (0,) for x in out]


def _decoy():
    return central(E(b"decoy.txt", b"", 0), 0, b"", 0)


def decoys():
    d = _decoy()
    stored = E(b"data.bin", b"head" + d + b"tail", 0)
    return [("in_name", build([E(b"a", b"A"), E(b"x" + d, b"B"), E(b"c", b"C")])),
            ("in_extra", build([E(b"a", b"A"), E(b"b", b"B", cextra=struct.pack("<HH", 0x9999, len(d)) + d), E(b"c", b"C")])),
            ("in_comment", build([E(b"a", b"A"), E(b"b", b"B", comment=d), E(b"c", b"C")])),
            ("in_stored_data", build([E(b"a", b"A"), stored, E(b"c", b"C")])),
            ("in_stored_data_prefixed", build([E(b"a", b"A"), stored, E(b"c", b"C")], prefix=b"junk" * 9)),
            ("in_span_behind_the_records", build([E(b"a", b"A"), E(b"c", b"C")], after_cd=d + b"pad"))]


def prefix_suffix():
    es = [E(b"p/a", blob(400, 1)), E(b"p/b", blob(50, 2), 0), E(b"p/", method=0)]
    return [("prefix%d" % n, build(es, prefix=blob(n, 9).replace(b"PK", b"pk"))) for n in (1, 7, 4096)] + [
        ("archive_comment", build(es, comment=b"a comment behind the end record")),
        ("prefix_and_comment", build(es, prefix=b"#!/bin/sh\n", comment=b"tail"))]


def _z64(usize=None, csize=None, hoff=None, tail=b""):
    body = b"".join(struct.pack("<Q", v) for v in (usize, csize, hoff) if v is not None) + tail
    return struct.pack("<HH", 1, len(body)) + body


def zip64_cases():
    data = blob(600, 6)
    st = deflate(data)
    first = E(b"first", b"12345", 0)  # 5 + 35 bytes in front: the second entry's header is at 40
    hoff = 30 + 5 + 5
    other = struct.pack("<HH", 0x5455, 5) + b"\x01abcd"
    out = [("create_layout", zip_oracle.create_archive([("a", data), ("b/c", b""), ("d", blob(70))]), 0),
           ("zip64_end_record", build([first, E(b"z", data)], zip64={}), 0),
           ("usize_only", build([first, E(b"z", data, c_usize=0xFFFFFFFF, cextra=_z64(usize=len(data)))]), 0),
           ("csize_only", build([first, E(b"z", data, c_csize=0xFFFFFFFF, cextra=_z64(csize=len(st)))]), 0),
           ("hoff_only", build([first, E(b"z", data, c_hoff=0xFFFFFFFF, cextra=_z64(hoff=hoff))]), 0),
           ("all_three", build([first, E(b"z", data, c_usize=0xFFFFFFFF, c_csize=0xFFFFFFFF, c_hoff=0xFFFFFFFF,
                                         cextra=_z64(len(data), len(st), hoff))]), 0),
           # the reference reads the field header at the FIRST extra field whatever its cursor says: the zip64 field
           # behind another one is never seen, the ff-filled sizes stay
           ("zip64_not_first", build([first, E(b"z", data, c_usize=0xFFFFFFFF,
                                               cextra=other + _z64(usize=len(data)))]), None),
           ("zip64_truncated", build([first, E(b"z", data, c_usize=0xFFFFFFFF, c_csize=0xFFFFFFFF,
                                               cextra=_z64(usize=len(data)))]), ARCHIVE_EOF),
           ("zip64_field_of_4", build([first, E(b"z", data, c_usize=0xFFFFFFFF, cextra=_z64(tail=b"1234"))]),
            ARCHIVE_EOF)]
    return out


def names():
    d = blob(64, 8)
    utf = "näme/€.txt".encode("utf-8")
    cp = b"caf\x82/\x9b\xe1.txt"  # valid CP437, invalid UTF-8
    n65 = bytearray(b"a" * 80)
    out = [("utf8_flag_set", build([E(utf, d), E(cp, d, flags=0x0800)]), 0),
           ("utf8_flag_clear", build([E(utf, d, flags=0)]), 0),
           ("cp437", build([E(cp, d, flags=0), E(b"plain", d, flags=0)]), 0),
           ("two_byte_lead_c1", build([E(b"a\xc1\x80b", d, flags=0)]), 0),
           ("lead_without_tail", build([E(b"ab\xe2\x82", d, flags=0)]), 0),
           ("tail_too_long", build([E(b"a\xc3\xa4\xa4b", d, flags=0)]), 0),
           ("four_byte", build([E("a\U0001F600b".encode("utf-8"), d, flags=0)]), 0),
           ("f8", build([E(b"a\xf8\x80\x80\x80\x80", d, flags=0)]), 0)]
    for at in (0, 63, 64, len(n65) - 1):
        n = bytearray(n65)
        n[at] = 0xFF
        out.append(("bad_lead_at%d" % at, build([E(bytes(n), d, flags=0)]), 0))
        n = bytearray(n65)
        n[at] = 0xC3  # a lead whose continuation byte is an ASCII letter (or the end of the name)
        out.append(("lead_at%d" % at, build([E(bytes(n), d, flags=0)]), 0))
    out += [("trailing_slash", build([E(b"d1/", method=0), E(b"d1/f", d)]), 0),
            ("dos_dir_bit", build([E(b"d2", method=0, external=0x10), E(b"f", d)]), 0),
            ("unix_dir_bit", build([E(b"d3", method=0, external=(0o040755 << 16)), E(b"f", d, external=0o100644 << 16)]), 0)]
    for i, n in enumerate([b"/abs", b"../up", b"..\\up", b"a/../b", b"a\\..\\b", b"x" * 62 + b"/../y", b"x" * 61 + b"/../y",
                           b"/"]):
        out.append(("unsafe_file%d" % i, build([E(b"ok", d), E(n, d), E(b"after", d, 0)]), UNSAFE_PATH))
        out.append(("unsafe_dir%d" % i, build([E(b"ok", d), E(n + b"/", method=0), E(b"after", d, 0)]), UNSAFE_PATH))
    out.append(("safe_near_misses", build([E(n, d) for n in [b"..", b"a/..", b"a/..b/c", b"...", b"a/.../b", b"..a/b"]]), 0))
    return out


def open_statuses():
    """(id, image, status): every status of zh_zip_open"""
    es = [E(b"a", b"A" * 50), E(b"b", blob(300)), E(b"c", b"C", 0)]
    good = build(es)

    def with_entry(i, **kw):
        x = [dict(e) for e in es]
        x[i].update(kw)
        return build(x)
    z_bad = build(es, zip64={"sig": 0x06064B51})
    return [("no_eocd", good[:-22] + b"\0" * 22, ARCHIVE_EOF), ("empty", b"", ARCHIVE_EOF), ("short", b"PK\5\6", ARCHIVE_EOF),
            ("disk_number", build(es, disk=1), UNSUPPORTED), ("start_disk", build(es, start_disk=1), UNSUPPORTED),
            ("record_count", build(es, on_disk=2), UNSUPPORTED),
            ("zip64_locator_disk", build(es, zip64={"loc_disk": 1}), UNSUPPORTED),
            ("zip64_disk_count", build(es, zip64={"disks": 2}), UNSUPPORTED),
            ("bad_sig_record0", with_entry(0, c_sig=0x02014B51), CENTRAL_HEADER),
            ("bad_sig_last", with_entry(2, c_sig=0x02014B51), CENTRAL_HEADER),
            ("bad_sig_zip64_end", z_bad, CENTRAL_HEADER),
            ("method", with_entry(1, c_method=9), METHOD), ("file_disk", with_entry(1, disk=3), DISK_NUMBER),
            ("duplicate", build(es + [E(b"b", b"again")]), DUPLICATE),
            ("central_size", build(es, cd_size_delta=-5), CENTRAL_SIZE),
            ("count_too_large", build(es, num=4, on_disk=4), None)]


def precedence():
    a, b, c, d = E(b"a", b"A"), E(b"b", b"B"), E(b"c", b"C"), E(b"d", b"D")
    dup = E(b"a", b"again")
    bad = dict(c_method=9)
    trunc = dict(c_usize=0xFFFFFFFF, c_csize=0xFFFFFFFF, cextra=_z64(usize=1))
    return [("method_before_dup", build([a, dict(b, **bad), dup, d]), METHOD),
            ("method_at_dup", build([a, b, dict(dup, **bad), d]), METHOD),
            ("dup_before_method", build([a, b, dup, dict(d, **bad)]), DUPLICATE),
            ("dup_with_truncated_zip64", build([a, b, dict(dup, **trunc), d]), DUPLICATE),
            ("truncated_zip64_alone", build([a, b, dict(c, **trunc), d]), ARCHIVE_EOF),
            ("two_failures", build([a, dict(b, disk=1), dict(c, **bad), d]), DISK_NUMBER),
            ("open_failure_and_bad_entry", build([a, dict(b, crc=1), dict(c, **bad)]), METHOD),
            ("central_size_before_later_dup", build([a, b, dup], cd_size_delta=-60), CENTRAL_SIZE)]


def entry_statuses():
    """(id, image, archive status): one damaged file entry in an otherwise good archive"""
    data = blob(2000, 11)
    st = deflate(data)
    broken = bytearray(st)
    broken[len(st) // 2] ^= 0x5A
    broken[len(st) // 2 + 1] ^= 0xA5
    pre, post = E(b"pre", blob(100, 1), 0), E(b"post", blob(1500, 2))

    def one(**kw):
        return build([pre, E(b"x", data, **kw), post])
    out = [("local_sig", one(l_sig=0x04034B51), FILE_HEADER),
           ("local_method_0", one(l_method=0), None),  # the stream's bytes as they are: the CRC decides
           ("local_method_8", one(), 0),
           ("local_method_9", one(l_method=9), METHOD),
           ("central_0_local_8", build([pre, E(b"x", data, 8, c_method=0), post]), 0),
           ("data_past_image", one(c_csize=1 << 20), ARCHIVE_EOF),
           ("hoff_past_image", one(c_hoff=1 << 24), ARCHIVE_EOF),
           ("crc_stored", build([pre, E(b"x", data, 0, crc=5), post]), CRC),
           ("crc_deflated", one(crc=zlib.crc32(data) ^ 1), CRC),
           ("damaged_stream", one(stream=bytes(broken)), None),
           ("cut_stream", one(stream=st[:len(st) // 2]), None),
           ("usize_understated", one(c_usize=100), 0),  # the retry path
           ("usize_understated_0", one(c_usize=0), 0),
           ("usize_overstated", one(c_usize=len(data) + 5000), 0),
           ("usize_overstated_much", one(c_usize=0xFFFFFFF0), 0),
           ("empty_deflated", build([pre, E(b"x", b"", 8), post]), 0),
           ("empty_stored", build([pre, E(b"x", b"", 0), post]), 0),
           ("two_bad", build([pre, E(b"x", data, crc=1), E(b"y", data, l_method=12), post]), CRC)]
    return out


ALIGN_LENS = (0, 1, 15, 16, 17, 4097)


def alignment():
    """(id, image): one stored and one deflated archive in which, for each of the lengths 0, 1, 15, 16, 17 and 4097,
    an entry's data start at every address mod 16 of the image.  Each entry's local extra field is sized from the
    running offset, so that the residues do not depend on what the names and streams before it happen to weigh; the
    function itself asserts, on the image it built, that all 16 occur per length and method."""
    out = []
    for method in (0, 8):
        prefix = b"\0" * (3 * method)
        es = []
        at = len(prefix)
        for k, n in enumerate(ALIGN_LENS):
            for want in range(16):
                name = b"m%d/n%d/r%02d" % (method, n, want)
                data = blob(n, want + k)
                stream = deflate(data) if method == 8 else data
                start = at + 30 + len(name) + 4  # the data's address with an extra field of its header alone
                pad = (want - start) % 16
                es.append(E(name, data, method, lextra=struct.pack("<HH", 0x4141, pad) + b"." * pad))
                at = start + pad + len(stream)
        image = build(es, prefix=prefix)
        seen = {n: set() for n in ALIGN_LENS}
        for e in es:  # the addresses, read back from the image
            lh = image.index(struct.pack("<HH", len(e["name"]), len(e["lextra"])) + e["name"]) - 26
            assert image[lh:lh + 4] == b"PK\3\4"
            seen[len(e["data"])].add((lh + 30 + len(e["name"]) + len(e["lextra"])) % 16)
        assert all(seen[n] == set(range(16)) for n in ALIGN_LENS), seen
        out.append(("method%d" % method, image))
    return out


def copy_shifts(eng, image, n=4097):
    """the distances mod 16 between where the stored entries of n bytes lie in the image and where they lie in the
    reader's block (whose start is 16-byte aligned on the device): the shifts the stored copy's gather runs at"""
    readers, sts = eng.open_zips([image])
    try:
        block = readers[0].data
        out = set()
        for i, e in enumerate(readers[0].entries):
            data = readers[0].contents(i)
            if len(data) == n:
                assert image.count(data) == 1 and block.count(data) == 1
                out.add((image.index(data) - block.index(data)) % 16)
        return out
    finally:
        readers[0].close()


_MUTATIONS = ["none", "none", "none", "none", "none", "none", "crc", "local_sig", "method", "cut", "dup", "disk", "cd_size",
              "stream", "usize", "unsafe", "eocd", "prefix"]


def random_images(seed, n):
    """n small archives from a seeded generator, about half of them damaged"""
    rng = random.Random(seed)
    out = []
    for t in range(n):
        es = []
        for i in range(rng.randrange(0, 9)):
            k = rng.choice([0, 1, 17, 300, 2500])
            name = b"t%d/%s%d" % (t, rng.choice([b"f", b"g" * 40, b"caf\x82"]), i)
            if rng.random() < 0.15:
                es.append(E(name + b"/", method=0, flags=rng.choice([0, 0x800])))
            else:
                es.append(E(name, blob(k, t + i), rng.choice([0, 8, 8]), flags=rng.choice([0, 0x800])))
        kw = {}
        m = rng.choice(_MUTATIONS) if rng.random() < 0.75 else "none"
        files = [e for e in es if not e["name"].endswith(b"/")]
        if m in ("crc", "local_sig", "method", "stream", "usize", "unsafe", "dup", "disk") and not files:
            m = "none"
        if m != "none" and files:
            e = rng.choice(files)
            if m == "crc":
                e["crc"] = 7
            elif m == "local_sig":
                e["l_sig"] = 0
            elif m == "method":
                e[rng.choice(["c_method", "l_method"])] = 12
            elif m == "stream" and e["method"] == 8 and len(e["data"]) > 100:
                s = bytearray(deflate(e["data"]))
                s[len(s) // 2] ^= 0xFF
                e["stream"] = bytes(s)
            elif m == "usize":
                e["c_usize"] = rng.choice([0, 3, len(e["data"]) + 100])
            elif m == "unsafe":
                e["name"] = rng.choice([b"../", b"/", b"q/../"]) + e["name"]
            elif m == "dup":
                # Two records with one raw CP437 name are no test case: the duplicate check holds the RAW name against
                # the CONVERTED paths (ziparchives.nim:314, zh_zip_open), so it misses them, and then the referees part
                # -- the reference's table keeps one record, zh_zip_open (whose results are not this call's to change)
                # keeps both.  With the language-encoding flag the name is kept as it is and the duplicate is seen.
                if any(c >= 0x80 for c in e["name"]):
                    e["flags"] = 0x0800
                es.append(dict(e))
            elif m == "disk":
                e["disk"] = 2
        if m == "cd_size":
            kw["cd_size_delta"] = -rng.randrange(1, 40)
        if m == "eocd":
            kw[rng.choice(["disk", "start_disk"])] = 1
        if m == "prefix":
            kw["prefix"] = b"\x7f" * rng.randrange(1, 50)
        img = build(es, **kw)
        if m == "cut":
            img = img[:rng.randrange(0, len(img))]
        out.append(img)
    return out


# ---- the referees ----
def _unsafe(path):  # internal.nim:294-302
    return (path.startswith(b"/") or path.startswith(b"../") or path.startswith(b"..\\") or b"/../" in path
            or b"\\..\\" in path)


def _code(e):
    if e.status >= 0:
        return e.status
    return next(v for k, v in _MESSAGES.items() if str(e).startswith(k))


_expected = {}
U64 = (1 << 64) - 1


def expected(image):
    """(archive status, entries | None, [(entry status, bytes | None)] | None) of the serial reference"""
    image = bytes(image)
    if image in _expected:
        return _expected[image]
    try:
        r = zip_oracle.open_archive(image)
    except OracleError as e:
        _expected[image] = (_code(e), None, None)
        return _expected[image]
    except struct.error:  # (a field that points outside the image, read without a check)
        _expected[image] = (ARCHIVE_EOF, None, None)
        return _expected[image]
    entries, results = [], []
    size = len(image)
    recs = list(r.records.values())
    unsafe = any(_unsafe(x["path"]) for x in recs)
    status = UNSAFE_PATH if unsafe else 0
    for x in recs:
        e = dict(x, path=x["path"].decode("utf-8", "surrogateescape"))
        for k in ("compressed_size", "header_offset"):  # what no image can hold is kept as -1 (zh_zip_open)
            if e[k] > size:
                e[k] = U64
        entries.append(e)
        if x["is_directory"]:
            results.append((0, b""))
        elif unsafe:
            results.append((UNSAFE_PATH, None))
        else:
            try:
                results.append((0, zip_oracle.extract_file(r, x["path"])))
            except OracleError as err:
                results.append((_code(err), None))
            except struct.error:
                results.append((ARCHIVE_EOF, None))
            if results[-1][0] and not status:
                status = results[-1][0]
    _expected[image] = (status, entries, results)
    return _expected[image]


def alone(eng, image):
    """(open status, entries, [(status, bytes)] of the file records) of Engine.open_zip / extract_batch"""
    try:
        r = eng.open_zip(image)
    except ZippyError as e:
        return e.status, None, None
    try:
        idx = [i for i, e in enumerate(r.entries) if not e["is_directory"]]
        outs, sts = r.extract_batch(idx) if idx else ([], [])
        return 0, r.entries, dict(zip(idx, zip(sts, outs)))
    finally:
        r.close()


_ZIP_CODES = {0, ARCHIVE_EOF, FILE_HEADER, METHOD, CRC, UNSAFE_PATH}


def check_batch(eng, images, want=None, close_order=None, second_referee=True):
    """Open `images` in ONE call and hold every archive status, every field of every entry, every entry status and
    every extracted byte against the two referees (and against `want`, the statuses the case was built for; None:
    whatever the referees say).  Where the oracle's decoder rejects a stream, its code is the codec's own: there the
    second referee's code is the one to equal.  -> the statuses"""
    images = [bytes(b) for b in images]
    readers, sts = eng.open_zips(images)
    try:
        assert len(readers) == len(sts) == len(images)
        for t, image in enumerate(images):
            st, entries, results = expected(image)
            tag = "image %d" % t
            if want is not None and want[t] is not None:
                assert st == want[t], "%s: the reference says %d, built for %d" % (tag, st, want[t])
            second = alone(eng, image) if second_referee else None
            if entries is None:
                assert sts[t] == st, "%s: status %d, the reference says %d" % (tag, sts[t], st)
                assert readers[t] is None
                if second:
                    assert second[0] == st
                continue
            r = readers[t]
            assert r is not None, "%s: no reader, status %d" % (tag, sts[t])
            assert r.entries == entries, tag
            if second:
                assert second[0] == 0 and second[1] == entries, tag
            got = [(r.entry_status(i), r.contents(i)) for i in range(len(entries))]
            block = r.data
            first_bad = 0
            for i, (e, (est, data)) in enumerate(zip(entries, results)):
                where = "%s entry %d (%r)" % (tag, i, e["path"])
                if second and not e["is_directory"] and st != UNSAFE_PATH:
                    assert got[i] == second[2][i], where
                if est in _ZIP_CODES:
                    assert got[i] == (est, data), "%s: status %d, the reference says %d" % (where, got[i][0], est)
                else:
                    assert got[i][0] not in (0, CRC) and got[i][1] is None, where
                if got[i][0] and not e["is_directory"] and not first_bad:
                    first_bad = got[i][0]
                if got[i][0] == 0 and data and e["uncompressed_size"] == len(data):
                    assert data in block, where  # (an entry decoded again on its own lies outside the block)
            assert sts[t] == (UNSAFE_PATH if st == UNSAFE_PATH else first_bad), tag
            if all(x[0] in _ZIP_CODES for x in results):
                assert sts[t] == st, tag
            assert len(block) % 8 == 0 and (st != UNSAFE_PATH or block == b"")
    finally:
        order = list(range(len(readers))) if close_order is None else close_order
        for t in order:
            if readers[t] is not None:
                readers[t].close()
    return sts


def dump(directory):
    """the status and precedence cases as files (for the stand-alone sanitizer driver): NAME.zip + expected.txt"""
    os.makedirs(directory, exist_ok=True)
    lines = []
    for name, image, _ in open_statuses() + precedence() + entry_statuses() + names() + geometry() + zip64_cases():
        with open(os.path.join(directory, name + ".zip"), "wb") as f:
            f.write(image)
        lines.append("%s.zip %d" % (name, expected(image)[0]))
    with open(os.path.join(directory, "expected.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(lines)
