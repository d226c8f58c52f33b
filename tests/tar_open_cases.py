"""Shared by tests/test_emu_tar_open_batch.py and tests/test_gpu_tar_open_batch.py: hand-made and tarfile-made tarball
images, and the check of zh_tar_open_batch (Engine.open_tars) against its two referees -- oracle/tar_oracle.py's
open_tarball (tarballs.nim restated) and Engine.open_tar on every image by itself."""
import gzip
import io
import random
import tarfile

from oracle import ZippyError as OracleError
from oracle import tar_oracle
from zippy_amd.common import ZippyError

INVALID_BUFFER, ARCHIVE_EOF, HEADER_TYPE, UNSAFE_PATH, TAR_NUMBER = 13, 23, 34, 35, 36
CHECKSUM, SIZE = 8, 9

_MESSAGES = {"Invalid buffer, unable to uncompress": INVALID_BUFFER, "Unexpected EOF, invalid archive?": ARCHIVE_EOF,
             "Path not allowed": UNSAFE_PATH, "Unsupported header type": HEADER_TYPE, "invalid octal digit": TAR_NUMBER}


# ---- images by hand ----
def header(name=b"", size=0, typeflag=b"0", mode=b"0000644\0", mtime=b"14000000000\0", linkname=b"",
           magic=b"ustar\0" + b"00", prefix=b"", size_field=None):
    """One 512-byte header; size_field replaces the 12 bytes of the size field."""
    h = bytearray(512)
    h[0:len(name)] = name
    h[100:100 + len(mode)] = mode
    h[108:116] = b"0000000\0"
    h[116:124] = b"0000000\0"
    sf = size_field if size_field is not None else b"%011o\0" % size
    h[124:124 + len(sf)] = sf
    h[136:136 + len(mtime)] = mtime
    h[156:157] = typeflag
    h[157:157 + len(linkname)] = linkname
    h[257:257 + len(magic)] = magic
    h[345:345 + len(prefix)] = prefix
    h[148:156] = b"        "
    h[148:156] = b"%06o\0 " % sum(h)
    return bytes(h)


def entry(data=b"", **kw):
    return header(size=len(data), **kw) + data + bytes(-len(data) % 512)


def chain(n, tag=b"e"):
    """n headers of empty entries"""
    return b"".join(header(name=tag + b"%d" % i) for i in range(n))


END = bytes(1024)  # the two zero blocks a writer ends with (headers without a name: walked, not reported)


def long_name(path, name=b"././@LongLink"):
    """a GNU 'L' block whose contents are the path"""
    return entry(path, name=name, typeflag=b"L")


def blob(n, seed=1):
    return bytes((i * 131 + seed * 7 + (i >> 7)) & 0xFF for i in range(n))


def gz(image, level=6):
    return gzip.compress(image, level, mtime=0)


def tarfile_image(fmt, members, mode="w:"):
    """members: (name, contents | None for a directory | ('link', target))"""
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode=mode, format=fmt) as tf:
        for name, what in members:
            info = tarfile.TarInfo(name)
            info.mtime = 1600000000
            if what is None:
                info.type, info.mode = tarfile.DIRTYPE, 0o755
                tf.addfile(info)
            elif isinstance(what, tuple):
                info.type, info.linkname = tarfile.SYMTYPE, what[1]
                tf.addfile(info)
            else:
                info.size, info.mode = len(what), 0o644
                tf.addfile(info, io.BytesIO(what))
    return buf.getvalue()


MEMBERS = [("dir", None), ("dir/a.txt", b"alpha"), ("dir/link", ("link", "a.txt")), ("dir/" + "n" * 120, blob(700)),
           ("p" * 90 + "/" + "q" * 60 + "/r.bin", blob(513, 2)), ("dir/empty", b""),
           ("x" * 150 + "/" + "y" * 150 + "/z", b"deep")]


def good_images():
    return [tarfile_image(tarfile.USTAR_FORMAT, MEMBERS[:3] + MEMBERS[4:6]), tarfile_image(tarfile.GNU_FORMAT, MEMBERS),
            tarfile_image(tarfile.PAX_FORMAT, MEMBERS)]


# ---- the cases of the issue, as lists of (id, image) ----
def doubling_chains():
    ns = [1, 2, 3] + [n for k in range(2, 12) for n in ((1 << k) - 1, 1 << k, (1 << k) + 1)]
    return [("chain%d" % n, chain(n)) for n in sorted(set(ns))]


def doubling_shapes():
    return [("one_block", header(name=b"only")),
            ("big_first_jump", entry(blob(10 * 512 - 7), name=b"big") + chain(3)),
            ("big_first_jump_to_end", entry(blob(9 * 512), name=b"big")),
            ("empty_gzip", gz(b""))]


def decoys():
    inner = (entry(b"x", name=b"/etc/passwd") + entry(b"y", name=b"a/../../b") + entry(b"z", name=b"hard", typeflag=b"1")
             + header(name=b"bad", size_field=b"00000000008\0") + chain(5, b"inner") + END)
    nines = b"9" * 2048
    eights = (b"8" * 512) * 3
    return [("inner_tarball", entry(inner, name=b"inner.tar") + entry(b"after", name=b"after") + END),
            ("nines", entry(nines, name=b"nines") + entry(eights, name=b"eights") + chain(2) + END),
            ("inner_tarball_unaligned_tail", entry(inner + b"tail", name=b"inner.tar") + chain(1))]


def walk_semantics():
    a, b = tarfile_image(tarfile.USTAR_FORMAT, MEMBERS[:3]), tarfile_image(tarfile.GNU_FORMAT, MEMBERS[3:5])
    v7 = entry(b"old", name=b"v7file", magic=b"", prefix=b"ignored/prefix")
    gnu_magic = entry(b"gnu", name=b"gnufile", magic=b"ustar  \0", prefix=b"not/a/prefix")
    seams = b"".join(entry(b"s", name=n, prefix=p) for p, n in [
        (b"pre", b"name"), (b"pre/", b"name"), (b"pre", b"/name"), (b"pre/", b"/name"), (b"", b"name"),
        (b"p" * 155, b"n" * 100), (b"p" * 154 + b"/", b"/" + b"n" * 99), (b"a/b/c", b"d/e")])
    links = (entry(name=b"ln", typeflag=b"2", linkname=b"target/of/link") + entry(name=b"ln100", typeflag=b"2",
             linkname=b"t" * 100) + entry(name=b"d/", typeflag=b"5", mode=b"0000755\0") + entry(b"nul", name=b"nulflag",
             typeflag=b"\0"))
    skipped = b"".join(entry(b"17 path=hello\n", name=b"hdr", typeflag=t) for t in [b"g", b"x", b"A", b"K", b"S", b"Z"])
    ln = b"long/" + b"n" * 150 + b"/name.txt"
    longs = long_name(ln + b"\0") + entry(b"payload", name=b"short")
    return [
        ("zero_blocks_in_the_middle", a + b), ("three_concatenated", a + b + a),
        ("v7_and_gnu_magic", v7 + gnu_magic + END), ("prefix_seams", seams + END), ("links_and_dirs", links + END),
        ("skipped_types", skipped + entry(b"real", name=b"real") + END), ("gnu_long_name", longs + END),
        ("long_name_600", long_name(b"d/" * 299 + b"ab") + entry(b"p", name=b"s") + END),
        ("L_then_L", long_name(b"first/long\0") + long_name(b"second/long\0") + entry(b"p", name=b"short") + END),
        ("L_of_size_0", entry(b"", name=b"././@LongLink", typeflag=b"L") + entry(b"p", name=b"keeps/its/name") + END),
        ("L_as_last_header", entry(b"p", name=b"first") + long_name(b"dangling\0")),
        ("L_run_with_empty_names", long_name(b"one\0") + long_name(b"two\0", name=b"") * 3
         + long_name(b"three\0", name=b"") + entry(b"p", name=b"short") + entry(b"q", name=b"after") + END),
        ("L_run_from_the_start", long_name(b"never\0", name=b"") * 4 + entry(b"p", name=b"plain") + END),
        ("L_run_behind_an_empty_L", entry(b"", name=b"x", typeflag=b"L") + long_name(b"dead\0", name=b"") * 2
         + entry(b"p", name=b"plain2") + END),
        ("L_run_long", long_name(b"head\0") + long_name(b"mid\0", name=b"") * 70 + entry(b"p", name=b"") + chain(2)),
        ("long_name_for_a_nameless_header", long_name(b"named/by/L\0") + entry(b"p", name=b"") + END),
        ("unaligned_tail_not_reached", entry(b"x" * 100, name=b"short")[:512 + 100]),
        ("safe_near_misses", b"".join(entry(b"", name=n) for n in [b"..", b"a/..", b"a/..b/c", b"...", b"a/.../b",
                                                                   b"..a/b", b"a\\..", b".\\..\\"[:3] + b"x"]) + END),
    ]


_UNSAFE_NAMES = [b"/abs", b"../up", b"..\\up", b"a/../b", b"a\\..\\b", b"ab/../c", b"abc/../d", b"abcd/../e", b"/"]
_UNSAFE_JOINS = [(b"/abs", b"x"), (b"..", b"x"), (b"a/..", b"b"), (b"a", b"../b"), (b"..\\x", b"y"),
                 (b"a\\..\\b", b"c"), (b"p" * 152 + b"/..", b"q"), (b"a\\..\\", b"b")]


def statuses():
    """(id, image, status): every status, to be put between neighbours that open"""
    good = entry(b"ok", name=b"ok") + END
    out = [("len0", b"", INVALID_BUFFER), ("len1", b"\x1f", INVALID_BUFFER), ("len1_plain", b"a", INVALID_BUFFER),
           ("gzip17", gz(good)[:17], INVALID_BUFFER), ("gzip2", b"\x1f\x8b", INVALID_BUFFER)]
    g = bytearray(gz(good))
    g[-8] ^= 0x55
    out.append(("gzip_crc", bytes(g), CHECKSUM))
    for delta in (-1, 1, 5000):
        g = bytearray(gz(good * 3))
        isize = int.from_bytes(g[-4:], "little") + delta
        g[-4:] = isize.to_bytes(4, "little")
        out.append(("gzip_isize%+d" % delta, bytes(g), SIZE))
    out += [("len_not_512", good + b"x" * 100, ARCHIVE_EOF), ("len_511", good[:511], ARCHIVE_EOF),
            ("size_past_end", header(name=b"big", size=513) + bytes(512), ARCHIVE_EOF),
            ("size_past_end_huge", header(name=b"huge", size_field=b"77777777777\0"), ARCHIVE_EOF),
            ("gz_size_past_end", gz(header(name=b"big", size=1)), ARCHIVE_EOF),
            ("mode8", entry(b"", name=b"m", mode=b"0000648\0") + END, TAR_NUMBER),
            ("size8", header(name=b"s", size_field=b"00000000008\0") + END, TAR_NUMBER),
            ("size9_after_blanks", header(name=b"s", size_field=b"   19      \0") + END, TAR_NUMBER),
            ("mtime8", entry(b"", name=b"t", mtime=b"1400000000" + b"8\0") + END, TAR_NUMBER),
            ("type1", entry(b"", name=b"hard", typeflag=b"1") + END, HEADER_TYPE),
            ("type3", entry(b"", name=b"chr", typeflag=b"3") + END, HEADER_TYPE),
            ("type7_behind_good", good[:1024] + entry(b"", name=b"cont", typeflag=b"7") + END, HEADER_TYPE)]
    for i, n in enumerate(_UNSAFE_NAMES):
        out.append(("unsafe_name%d" % i, entry(b"u", name=n) + END, UNSAFE_PATH))
        out.append(("unsafe_long%d" % i, long_name(n + b"\0") + entry(b"u", name=b"s") + END, UNSAFE_PATH))
    for i, (p, n) in enumerate(_UNSAFE_JOINS):
        out.append(("unsafe_join%d" % i, entry(b"u", name=n, prefix=p) + END, UNSAFE_PATH))
    for at in (0, 5, 6, 7, 8, 505, 508, 509, 510, 511, 512, 513, 1020, 1021):  # lane and 512-byte borders of a long name
        n = b"a" * at + (b"/../" if at else b"../") + b"b" * 30
        out.append(("unsafe_long_at%d" % at, long_name(n) + entry(b"u", name=b"s") + END, UNSAFE_PATH))
    return out


def statuses_fine():
    """(id, image): octal fields that are odd and still parse"""
    return [("size_blank", header(name=b"z", size_field=b"           \0") + END),
            ("size_two_runs", header(name=b"z", size_field=b" 0 8 9     \0") + END),
            ("size_no_nul", entry(b"x" * 8, name=b"z", size_field=b"000000000109") + END),
            ("mode_digit_in_byte_8", entry(b"", name=b"z", mode=b"00006449") + END)]


def precedence():
    """(id, image, status)"""
    bad_type, bad_path = entry(b"", name=b"t", typeflag=b"1"), entry(b"", name=b"../p")
    bad_num, ok = entry(b"", name=b"n", mode=b"0000009\0"), entry(b"fine", name=b"fine")
    return [
        ("type_then_path", ok + bad_type + bad_path + END, HEADER_TYPE),
        ("path_then_type", ok + bad_path + bad_type + END, UNSAFE_PATH),
        ("number_then_eof", bad_num + header(name=b"big", size=99999), TAR_NUMBER),
        ("path_then_number", bad_path + bad_num + END, UNSAFE_PATH),
        ("far_apart", chain(300) + bad_type + chain(300) + bad_path + bad_num, HEADER_TYPE),
        # two faults in one header
        ("number_before_eof", header(name=b"x", size=99999, mode=b"0000008\0"), TAR_NUMBER),
        ("number_before_path_and_type", entry(b"", name=b"/x", typeflag=b"1", mtime=b"9\0") + END, TAR_NUMBER),
        ("eof_before_path", header(name=b"/x", size=99999, typeflag=b"1"), ARCHIVE_EOF),
        ("path_before_type", entry(b"", name=b"/x", typeflag=b"1") + END, UNSAFE_PATH),
        ("long_path_before_type", long_name(b"../x") + entry(b"", name=b"s", typeflag=b"1") + END, UNSAFE_PATH),
        ("long_name_hides_unsafe_name", long_name(b"fine/name") + entry(b"", name=b"../x", typeflag=b"1") + END,
         HEADER_TYPE),
        ("partial_block_before_anything", ok + b"/x" + b"9" * 300, ARCHIVE_EOF),
        # a nameless header is checked for numbers and EOF only
        ("nameless_bad_type_is_fine", ok + entry(b"", name=b"", typeflag=b"1") + END, 0),
        ("nameless_bad_number", ok + entry(b"", name=b"", mode=b"8\0") + END, TAR_NUMBER),
        ("fault_behind_the_walk", ok + END + bad_type[:100], ARCHIVE_EOF),
    ]


def random_images(seed, n, gz_share):
    """n small images from a seeded generator: tarfile-made in the three formats, with 'L' names, links and
    directories, some damaged, a share of them gzipped"""
    rng = random.Random(seed)
    pool = blob(1 << 16, seed)
    out = []
    for t in range(n):
        members = []
        for i in range(rng.randrange(0, 12)):
            name = "t%d/%s" % (t, rng.choice(["f", "g" * 40, "h" * 101, "i" * 90 + "/" + "j" * 90])) + str(i)
            r = rng.random()
            if r < 0.1:
                members.append((name, None))
            elif r < 0.2:
                members.append((name, ("link", "to/" + "k" * rng.randrange(1, 90))))
            else:
                k = rng.choice([0, 1, 511, 512, 513, 3000])
                at = rng.randrange(len(pool) - k)
                members.append((name, pool[at:at + k]))
        try:
            img = tarfile_image(rng.choice([tarfile.USTAR_FORMAT, tarfile.GNU_FORMAT, tarfile.PAX_FORMAT]), members)
        except ValueError:  # a name USTAR cannot split
            img = tarfile_image(tarfile.GNU_FORMAT, members)
        img = img[:rng.choice([len(img), len(img), len(img), 512 * rng.randrange(0, 4) + rng.choice([0, 0, 7])])]
        r = rng.random()
        if r < 0.08 and len(img) >= 512:
            b = bytearray(img)
            b[rng.choice([0, 100, 106, 124, 134, 146, 156])] = rng.choice(b"89/1L\\x")
            img = bytes(b)
        out.append(gz(img, 1) if rng.random() < gz_share else img)
    return out


# ---- the check ----
_expected = {}


def expected(image):
    """(status, data, entries) of the serial reference, computed once per image"""
    image = bytes(image)
    if image not in _expected:
        try:
            data, entries = tar_oracle.open_tarball(image)
            _expected[image] = (0, data, entries)
        except OracleError as e:
            st = e.status
            if st < 0:
                st = next(v for k, v in _MESSAGES.items() if str(e).startswith(k))
            _expected[image] = (st, None, None)
    return _expected[image]


def alone(eng, image):
    """(status, data, entries) of Engine.open_tar on the image by itself"""
    try:
        r = eng.open_tar(image)
    except ZippyError as e:
        return e.status, None, None
    try:
        return 0, r.data, r.entries
    finally:
        r.close()


def check_batch(eng, images, want=None, close_order=None, second_referee=True):
    """Open `images` in ONE call and hold every status, every image and every field of every entry against the two
    referees (and against `want`, the statuses the case was built for).  -> the statuses"""
    images = [bytes(b) for b in images]
    readers, sts = eng.open_tars(images)
    try:
        assert len(readers) == len(sts) == len(images)
        for t, image in enumerate(images):
            st, data, entries = expected(image)
            assert sts[t] == st, "image %d: status %d, the reference says %d" % (t, sts[t], st)
            if want is not None:
                assert sts[t] == want[t], "image %d: status %d, built for %d" % (t, sts[t], want[t])
            if st:
                assert readers[t] is None
                if second_referee:
                    assert alone(eng, image)[0] == st
                continue
            assert readers[t].data == data
            assert readers[t].entries == entries, "image %d" % t
            for i, e in enumerate(entries):
                assert readers[t].contents(i) == data[e["offset"]:e["offset"] + e["size"]]
            if second_referee:
                assert (0, readers[t].data, readers[t].entries) == alone(eng, image)
    finally:
        order = list(range(len(readers))) if close_order is None else close_order
        for t in order:
            if readers[t] is not None:
                readers[t].close()
    return sts
