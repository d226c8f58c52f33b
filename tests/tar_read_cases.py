"""Shared by tests/test_emu_tar_read_batch.py and tests/test_gpu_tar_read_batch.py: tarball images made header by
header (tests/tar_open_cases.py's helpers), and the check of zh_tar_read_batch (Engine.read_tars) against
tests/tar_v1_reader_model.py (tarballs_v1.nim's openStreamImpl restated).  Where the model's decoder rejects an image,
the status to equal is the one Engine.uncompress_batch gives the same bytes.

A case is (id, image, format, status); status None: whatever the model says, DECODER: a status of the codec's.  The
model alone decides what is expected; `status` is what the case was built for."""
import gzip
import os
import random

import tar_open_cases as tc
import tar_v1_reader_model as tm
import tar_writer_model as wm
from tar_open_cases import END, blob, entry, gz, header
from zippy_amd.common import ZippyError

OK, ARGUMENT, TAR_FORMAT, TAR_OPEN, TAR_OPEN_MODE, TAR_EOF = 0, 22, 46, 47, 48, 49
CHECKSUM, SIZE, INVALID_BUFFER = 8, 9, 13
DETECT, PLAIN, GZIP = tm.TF_DETECT, tm.TF_UNCOMPRESSED, tm.TF_GZIP
DECODER = "decoder"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tarballs")


def fixture():
    with open(os.path.join(GOLDEN, "libressl-3.4.2.tar.gz"), "rb") as f:
        return f.read()


def good_images():
    return [entry(b"alpha" * 40, name=b"dir/a.txt") + entry(name=b"dir", typeflag=b"5") + entry(blob(700), name=b"b") + END,
            gz(entry(blob(1500, 3), name=b"s/one", mode=b"000600 \0") + entry(b"", name=b"s/two") + END)]


# ---- the families ----
CHAIN_LENGTHS = sorted(set([1, 2, 3] + [n for k in range(2, 12) for n in ((1 << k) - 1, 1 << k, (1 << k) + 1)]))
ZERO_RUNS = (1, 2, 20, 63, 64, 65)
MAX_BLOCKS = 8600


def chain(n, z=0, tag=b"e"):
    """n named headers of empty entries, z nameless (zero) blocks behind each"""
    return b"".join(header(name=tag + b"%d" % i) + bytes(512 * z) for i in range(n))


def chains():
    out = [("chain%d" % n, chain(n), DETECT, OK) for n in CHAIN_LENGTHS]
    # the same lengths with runs of z nameless blocks between the entries: every z that keeps the image under
    # MAX_BLOCKS (4.2 MiB; every length keeps z = 1 and 2, every z its lengths up to 2^7 + 1)
    out += [("chain%d_z%d" % (n, z), chain(n, z), DETECT, OK) for n in CHAIN_LENGTHS for z in ZERO_RUNS
            if n * (z + 1) <= MAX_BLOCKS]
    out += [("zeros%d" % n, bytes(512 * n), DETECT, OK) for n in [1, 2] + [(1 << k) + 1 for k in range(2, 12)]]
    out.append(("empty_uncompressed", b"", PLAIN, OK))
    return out


CHAIN_PAIRS = [(127, 129), (129, 127), (1, 2049), (2048, 3), (255, 256)]


def ends():
    last = header(name=b"last", size=700)  # its padded end, 512 + 1024, passes an image of 512 + 700 + n bytes
    return [("partial1", chain(2) + b"x", DETECT, TAR_EOF), ("partial511", chain(2) + b"x" * 511, DETECT, TAR_EOF),
            ("partial1_not_reached", last + blob(700) + b"x", DETECT, OK),
            ("partial511_not_reached", last + blob(700) + b"x" * 311, DETECT, OK),
            ("unpadded_last_entry", header(name=b"five", size=5) + b"12345", DETECT, OK),
            ("contents_one_byte_short", header(name=b"six", size=6) + b"12345", DETECT, TAR_EOF),
            ("contents_one_block_short", header(name=b"big", size=513) + bytes(512), DETECT, TAR_EOF),
            ("nameless_partial", chain(1) + bytes(100), DETECT, TAR_EOF),
            ("only_partial", b"abc", DETECT, TAR_EOF)]


def decoys():
    bad = header(name=b"looks/bad", size_field=b"0000000000 \0")
    three = header(name=b"in1") + header(name=b"in2", typeflag=b"5") + header(name=b"in3")
    garbage = header(name=b"", size_field=b"garbage!!!!\0", mtime=b"not a time\0", mode=b"rwxrwxrw")
    inner = three + bad + header(name=b"unfinished", size=99999)
    return [("nameless_size_is_not_jumped", header(name=b"", size=3 * 512) + three + END, DETECT, OK),
            ("nameless_size_then_bad", header(name=b"", size=512) + bad, DETECT, TAR_OPEN),
            ("nameless_garbage", chain(1) + garbage + chain(1, tag=b"f") + END, DETECT, OK),
            ("lookalikes_in_contents", entry(inner, name=b"inner.tar") + entry(b"after", name=b"after") + END, DETECT, OK),
            ("lookalikes_in_directory_contents", entry(inner, name=b"d", typeflag=b"5") + chain(2), DETECT, OK)]


def _numbers(field):
    """(tag, the 11 bytes of a size / mtime slice or the 6 of a mode slice, fine?)"""
    n = 6 if field == "mode" else 11
    d = {"size": b"00000002345", "mtime": b"12345670123", "mode": b"123456"}[field]
    return [("digits", d, True), ("0o", b"0o" + d[2:], True), ("0O", b"0O" + d[2:], True),
            ("underscores", d[:2] + b"_" + d[3:-2] + b"_" + d[-1:], True), ("underscore_first", b"_" + d[1:], True),
            ("only_underscores", b"_" * n, False), ("0o_underscores", b"0o" + b"_" * (n - 2), False),
            ("digit8", d[:-1] + b"8", False), ("digit9", b"9" + d[1:], False), ("8_in_the_middle", d[:3] + b"8" + d[4:], False),
            ("space_last", d[:-1] + b" ", False), ("space_middle", d[:3] + b" " + d[4:], False),
            ("space_first", b" " + d[1:], False), ("nul_last", d[:-1] + b"\0", False),
            ("nul_middle", d[:3] + b"\0" + d[4:], False), ("all_nul", bytes(n), False), ("all_spaces", b" " * n, False),
            ("o_without_0", b"o" + d[1:], False), ("0o_twice", b"0o0o" + d[4:], False), ("0x", b"0x" + d[2:], False)]


def _with_field(field, value):
    """a header whose `field` slice is `value`, with the contents its size field states (none if it does not parse)"""
    if field == "size":
        try:
            size = tm.parse_oct_int(value)
        except ValueError:
            size = 0
        return header(name=b"n", size_field=value + b"\0") + blob(size) + bytes(-size % 512)
    if field == "mtime":
        return header(name=b"n", mtime=value + b"\0")
    return header(name=b"n", mode=value + b" \0")


def number_parsing():
    out = []
    for field, bad in (("size", TAR_OPEN), ("mtime", TAR_OPEN), ("mode", TAR_OPEN_MODE)):
        for tag, value, fine in _numbers(field):
            want = OK if fine else bad
            out.append(("%s_%s" % (field, tag), chain(1) + _with_field(field, value) + chain(1, tag=b"f"), DETECT, want))
    out += [("size_small", chain(1) + entry(b"12345678", name=b"n", size_field=b"00000000010\0") + chain(1), DETECT, OK),
            ("size_0o_small", chain(1) + entry(b"12345678", name=b"n", size_field=b"0o0_0000_10\0") + chain(1), DETECT, OK),
            ("size_10_digits_and_space", entry(b"123", name=b"n", size_field=b"0000000003 \0"), DETECT, TAR_OPEN),
            ("size_byte_12_is_a_digit", entry(b"12345678", name=b"n", size_field=b"000000000107"), DETECT, OK),
            ("mode_seventh_byte_digit", entry(b"m", name=b"n", mode=b"0000644\0"), DETECT, OK),   # -> 0o64
            ("mode_v7", entry(b"m", name=b"n", mode=b"100664 \0"), DETECT, OK),                   # -> 0o100664
            ("mode_seventh_byte_8", entry(b"m", name=b"n", mode=b"00006448"), DETECT, OK),
            ("mtime_byte_12_is_a_digit", entry(b"m", name=b"n", mtime=b"140000000009"), DETECT, OK)]
    return out


def precedence():
    ok = entry(b"fine", name=b"fine")
    bs, bt, bm = b"0000000000 \0", b"1400000000 \0", b"00064 \0"
    return [("size_and_mode", ok + header(name=b"x", size_field=bs, mode=bm), DETECT, TAR_OPEN),
            ("mtime_and_mode", ok + header(name=b"x", mtime=bt, mode=bm), DETECT, TAR_OPEN),
            ("mode_alone", ok + header(name=b"x", mode=bm), DETECT, TAR_OPEN_MODE),
            ("mode_and_contents_past_end", ok + header(name=b"x", mode=bm, size=99999), DETECT, TAR_OPEN_MODE),
            ("mtime_and_contents_past_end", ok + header(name=b"x", mtime=bt, size=99999), DETECT, TAR_OPEN),
            ("contents_past_end_alone", ok + header(name=b"x", size=99999), DETECT, TAR_EOF),
            ("partial_block_before_numbers", ok + header(name=b"x", size_field=bs)[:300], DETECT, TAR_EOF),
            ("mode_then_size", ok + header(name=b"x", mode=bm) + header(name=b"y", size_field=bs), DETECT, TAR_OPEN_MODE),
            ("size_then_mode", ok + header(name=b"y", size_field=bs) + header(name=b"x", mode=bm), DETECT, TAR_OPEN),
            ("mode_then_eof_far_apart", chain(300) + header(name=b"x", mode=bm) + chain(300) + b"tail", DETECT,
             TAR_OPEN_MODE),
            ("eof_then_mode_far_apart", chain(300) + chain(40, 7) + header(name=b"big", size=10 ** 6)
             + header(name=b"x", mode=bm), DETECT, TAR_EOF),
            ("bad_header_not_reachable", entry(header(name=b"x", mode=bm) + header(name=b"y", size_field=bs),
                                               name=b"holds/them") + ok + END, DETECT, OK),
            ("bad_type_is_no_error", ok + entry(b"", name=b"hard", typeflag=b"1") + END, DETECT, OK),
            ("skipped_type_is_still_checked", ok + header(name=b"x", typeflag=b"x", mode=bm), DETECT, TAR_OPEN_MODE),
            ("skipped_type_past_end", ok + header(name=b"x", typeflag=b"L", size=3000), DETECT, TAR_EOF)]


def magic_and_join():
    def e(prefix, name=b"name", magic=b"ustar\0" + b"00", **kw):
        return entry(b"j", name=name, prefix=prefix, magic=magic, **kw)
    seams = [(b"pre", b"name"), (b"pre/", b"name"), (b"pre", b"/name"), (b"pre/", b"/name")]
    return [("ustar", e(b"pre/fix") + END, DETECT, OK), ("ustar_gnu", e(b"not/a/prefix", magic=b"ustar  \0") + END, DETECT, OK),
            ("ustar_byte_262", e(b"not/a/prefix", magic=b"ustar" + b"x00") + END, DETECT, OK),
            ("ustar_uppercase", e(b"not/a/prefix", magic=b"USTAR\0") + END, DETECT, OK),
            ("no_magic", e(b"ignored/prefix", magic=b"") + END, DETECT, OK),
            ("seams", b"".join(e(p, n) for p, n in seams) + e(b"", b"alone") + e(b"a/b/c", b"d/e") + e(b"/", b"/") + END,
             DETECT, OK),
            ("key256", e(b"p" * 155, b"n" * 100) + END, DETECT, OK),
            ("key255_two_slashes", e(b"p" * 154 + b"/", b"/" + b"n" * 99) + END, DETECT, OK),
            ("name100_no_prefix", e(b"", b"n" * 100, magic=b"") + END, DETECT, OK),
            ("prefix155_directory", e(b"q" * 155, b"d", typeflag=b"5") + END, DETECT, OK)]


def keys():
    def f(name, data, **kw):
        return entry(data, name=name, **kw)
    return [("backslashes", f(b"a\\b\\c", b"1") + f(b"n", b"2", prefix=b"p\\q") + f(b"\\", b"3") + END, DETECT, OK),
            ("backslash_and_slash_one_key", f(b"a\\b", b"first") + f(b"c", b"C") + f(b"a/b", b"second, longer") + END, DETECT, OK),
            ("repeated_key", f(b"k", b"1", mtime=b"00000000001\0") + f(b"m", b"M") + f(b"k", b"22", mtime=b"00000000002\0",
                                                                                       mode=b"000600 \0") + f(b"z", b"Z") + END, DETECT, OK),
            ("repeated_three_times", b"".join(f(b"k%d" % (i % 3), b"v%d" % i) for i in range(9)) + END, DETECT, OK),
            ("file_then_directory", f(b"k", b"file") + f(b"o", b"O") + f(b"k", b"", typeflag=b"5") + END, DETECT, OK),
            ("directory_then_file", f(b"k", b"", typeflag=b"5") + f(b"o", b"O") + f(b"k", b"file") + END, DETECT, OK),
            ("prefix_name_equals_name", f(b"p/n", b"by name") + f(b"n", b"by prefix", prefix=b"p") + END, DETECT, OK),
            ("seam_equals_name", f(b"n", b"1", prefix=b"p/") + f(b"/n", b"2", prefix=b"p") + f(b"p\\n", b"3") + END, DETECT, OK)]


def type_flags():
    ln = b"long/" + b"n" * 150 + b"/name.txt"
    out = [("file_0_and_nul", entry(b"zero", name=b"a") + entry(b"nul", name=b"b", typeflag=b"\0") + END, DETECT, OK),
           ("directory_with_everything", entry(blob(700), name=b"d", typeflag=b"5", mode=b"000755 \0") + chain(2), DETECT, OK),
           ("gnu_long_name", tc.long_name(ln + b"\0") + entry(b"payload", name=ln[:100]) + END, DETECT, OK)]
    for t in (b"1", b"2", b"L", b"x", b"g", b"Z", b"\xff", b"3", b"7", b" "):
        out.append(("type_%02x" % t[0], chain(1) + entry(b"17 path=hello\n", name=b"hdr", typeflag=t, linkname=b"to")
                    + chain(1, tag=b"f") + END, DETECT, OK))
    out += [("tarfile_%d" % i, img, DETECT, OK) for i, img in enumerate(tc.good_images())]
    return out


def formats():
    good = entry(b"ok", name=b"ok") + END
    g = gz(good)
    return [("detect_gzip", g, DETECT, OK), ("detect_plain", good, DETECT, OK),
            ("detect_1f_00", b"\x1f\0" + good[2:], DETECT, TAR_FORMAT), ("detect_1f_8a", b"\x1f\x8a" + g[2:], DETECT, TAR_FORMAT),
            ("detect_len0", b"", DETECT, TAR_FORMAT), ("detect_len1_1f", b"\x1f", DETECT, TAR_FORMAT),
            ("detect_len1", b"a", DETECT, TAR_EOF), ("detect_len2_1f_8b", b"\x1f\x8b", DETECT, DECODER),
            ("detect_len17", g[:17], DETECT, DECODER), ("detect_len18", g[:18], DETECT, DECODER),
            ("gzip_forced", g, GZIP, OK), ("gzip_forced_on_plain", good, GZIP, DECODER),
            ("gzip_forced_on_18_bytes", good[:18], GZIP, DECODER), ("gzip_forced_on_17_bytes", good[:17], GZIP, DECODER),
            ("gzip_forced_on_len0", b"", GZIP, DECODER), ("gzip_forced_on_len1", b"\x1f", GZIP, DECODER),
            ("plain_forced", good, PLAIN, OK), ("plain_forced_on_gzip", g, PLAIN, None),
            ("plain_forced_on_gzip_512", (g + bytes(512))[:512], PLAIN, None),
            ("plain_forced_on_1f_00", b"\x1f\0" + good[2:], PLAIN, OK), ("plain_forced_len1", b"\x1f", PLAIN, TAR_EOF)]


def gzips():
    good = entry(blob(3000, 5), name=b"g/data") + entry(b"", name=b"g/dir", typeflag=b"5") + END
    g = bytearray(gz(good))
    g[-8] ^= 0x55
    out = [("gz_empty", gz(b""), DETECT, OK), ("gz_crc", bytes(g), DETECT, CHECKSUM)]
    out += [("gz_level%d" % lv, gz(good, lv), DETECT, OK) for lv in (0, 1, 9)]
    for delta in (-1, 1, 5000):
        g = bytearray(gz(good))
        g[-4:] = (int.from_bytes(g[-4:], "little") + delta).to_bytes(4, "little")
        out.append(("gz_isize%+d" % delta, bytes(g), DETECT, SIZE))
    plain = gz(good)
    fname = plain[:3] + b"\x08" + plain[4:10] + b"libressl.tar\0" + plain[10:]
    out += [("gz_fname", fname, DETECT, OK), ("gz_truncated", plain[:len(plain) // 2], DETECT, DECODER),
            ("gz_truncated_trailer", plain[:-5], DETECT, DECODER), ("gz_of_partial", gz(good + b"x" * 100), DETECT, TAR_EOF),
            ("gz_of_bad_mode", gz(header(name=b"x", mode=b"00064 \0")), GZIP, TAR_OPEN_MODE),
            ("gz_unpadded_last_entry", gz(header(name=b"five", size=5) + b"12345"), DETECT, OK)]
    return out


ROUND_TRIP = [[("d", (b"", "5", 0)), ("d/a.txt", (b"alpha" * 50, "0", 1600000000)), ("d/empty", b""),
               ("deep/er/b.bin", (blob(70000, 4), "0", 7))],
              [("solo", (blob(513, 9), "0", 0o7777777777)), ("dir/with/bytes", (b"kept by the writer", "5", 5))]]


def written(entries):
    """what reading back an image writeTarball wrote of `entries` gives: [(key, kind, contents, mtime, mode)]"""
    out = []
    for path, contents, kind, mtime in wm.normalize(entries):
        head, tail = wm.split_path(path)
        key = tm.join(head, tail)
        out.append((key, kind, contents, mtime, 0o777) if kind == b"0" else (key, kind, b"", 0, 0))
    return out


def table_rows(table):
    return [(k, v["kind"], v["contents"], v["mtime"], v["mode"]) for k, v in table.items()]


def families():
    return [("chains", chains()), ("ends", ends()), ("decoys", decoys()), ("number_parsing", number_parsing()),
            ("precedence", precedence()), ("magic_and_join", magic_and_join()), ("keys", keys()),
            ("type_flags", type_flags()), ("formats", formats()), ("gzips", gzips())]


def all_cases():
    return [c for _, cs in families() for c in cs]


def random_images(seed, n):
    """n (image, format) pairs from a seeded generator, assembled from the families' pieces"""
    rng = random.Random(seed)
    small = [c for c in all_cases() if len(c[1]) <= 8192]
    names = [b"f", b"g" * 40, b"h\\i", b"d/e/f", b"n" * 100]
    out = []
    for t in range(n):
        r = rng.random()
        if r < 0.3:
            _, img, fmt, _ = rng.choice(small)
            out.append((img, fmt))
            continue
        parts = []
        for i in range(rng.randrange(0, 10)):
            k = rng.choice([0, 1, 511, 512, 513, 3000])
            kw = dict(name=rng.choice(names) + (b"%d" % rng.randrange(4) if rng.random() < 0.8 else b""),
                      typeflag=rng.choice([b"0", b"0", b"0", b"\0", b"5", b"2", b"x", b"L"]),
                      mode=rng.choice([b"000644 \0", b"0000644\0", b"100664 \0", b"0o_755 \0"]),
                      mtime=rng.choice([b"14000000000\0", b"0o123456701\0", b"00000000000 "]))
            if rng.random() < 0.3:
                kw.update(prefix=rng.choice([b"p", b"p/", b"q\\r"]), magic=rng.choice([b"ustar\0" + b"00", b"ustar  \0"]))
            if len(kw["name"]) > 100:
                kw["name"] = kw["name"][:100]
            parts.append(entry(blob(k, t + i), **kw) + bytes(512 * rng.choice([0, 0, 0, 1, 3])))
        img = b"".join(parts) + rng.choice([b"", END, END, bytes(10240)])
        m = rng.random()
        if m < 0.12 and len(img) >= 512:
            b = bytearray(img)
            b[rng.choice([0, 100, 105, 106, 124, 134, 135, 136, 146, 156, 262])] = rng.choice(b"89 _\0o/L")
            img = bytes(b)
        elif m < 0.2:
            img = img[:rng.randrange(0, len(img) + 1)]
        if rng.random() < 0.35:
            out.append((gzip.compress(img, rng.choice([0, 1, 6]), mtime=0), rng.choice([DETECT, DETECT, GZIP])))
        else:
            out.append((img, rng.choice([DETECT, DETECT, PLAIN])))
    return out


# ---- the check ----
_decoder = {}


def decoder_status(eng, image):
    if image not in _decoder:
        _decoder[image] = eng.uncompress_batch([image], 2)[1][0]
        assert _decoder[image] not in (OK, TAR_FORMAT, TAR_OPEN, TAR_OPEN_MODE, TAR_EOF)
    return _decoder[image]


def built_for(model_status, want):
    """is the model's verdict what the case was built for?  (the model has one verdict for every failure of the
    decoder: None; a case may name the codec's status it expects, all of which lie under ARGUMENT)"""
    if want is None:
        return True
    if model_status is None:
        return want == DECODER or 0 < want < ARGUMENT
    return model_status == want


def check_batch(eng, images, formats=None, want=None, close_order=None):
    """Open `images` in ONE call and hold every status, the key order, every field and every content byte against the
    model (and against `want`, the statuses the cases were built for).  -> the statuses"""
    images = [bytes(b) for b in images]
    readers, sts = eng.read_tars(images, formats)
    try:
        assert len(readers) == len(sts) == len(images)
        for t, image in enumerate(images):
            st, data, table = tm.expected(image, DETECT if formats is None else formats[t])
            tag = "image %d" % t
            if want is not None:
                assert built_for(st, want[t]), "%s: the model says %r, built for %r" % (tag, st, want[t])
            if table is None:
                if st is None:
                    st = decoder_status(eng, image)
                    assert want is None or want[t] in (None, DECODER, st), "%s: the decoder says %d" % (tag, st)
                assert sts[t] == st, "%s: status %d, the model says %d" % (tag, sts[t], st)
                assert readers[t] is None, tag
                continue
            r = readers[t]
            assert sts[t] == OK and r is not None, "%s: status %d, the model opens it" % (tag, sts[t])
            assert r.data == data, tag
            assert [e["path"] for e in r.entries] == list(table), tag
            for i, (key, v) in enumerate(table.items()):
                where = "%s entry %d (%r)" % (tag, i, key[:40])
                e = r.entries[i]
                assert e["typeflag"] == v["kind"] and e["linkname"] == b"", where
                for f in ("mode", "mtime", "offset", "size"):
                    assert e[f] == v[f], "%s: %s" % (where, f)
                assert r.contents(i) == v["contents"], where
    finally:
        order = list(range(len(readers))) if close_order is None else close_order
        for t in order:
            if readers[t] is not None:
                readers[t].close()
    return sts


def run_cases(eng, cases, alone=True, neighbours=True):
    """every case by itself, between two neighbours that open, and all in one call"""
    good = good_images()
    for name, image, fmt, want in cases:
        if alone:
            check_batch(eng, [image], [fmt], want=[want])
        if neighbours:
            sts = check_batch(eng, [good[0], image, good[1]], [DETECT, fmt, GZIP], want=[OK, want, OK])
            assert sts[0] == sts[2] == OK, name
    check_batch(eng, [c[1] for c in cases], [c[2] for c in cases], want=[c[3] for c in cases])


def with_error(status, fn):
    try:
        fn()
    except ZippyError as e:
        assert e.status == status, e.status
    else:
        raise AssertionError("no error %d" % status)


def dump(directory, cases):
    """cases as files (for the stand-alone sanitizer driver): NAME.tar + expected.txt, "NAME.tar FORMAT STATUS" a
    line; a decoder status is written as -1 (any status outside the archive layer's)"""
    os.makedirs(directory, exist_ok=True)
    lines = []
    for name, image, fmt, _ in cases:
        with open(os.path.join(directory, name + ".tar"), "wb") as f:
            f.write(image)
        st = tm.expected(image, fmt)[0]
        lines.append("%s.tar %d %d" % (name, fmt, -1 if st is None else st))
    with open(os.path.join(directory, "expected.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(lines)
