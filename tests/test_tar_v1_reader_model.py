"""CPU-only: tests/tar_v1_reader_model.py (tarballs_v1.nim's openStreamImpl restated, the referee of
zh_tar_read_batch) pinned four ways: against Python's tarfile, against tests/tar_writer_model.py (writeTarball
restated), on the reference's fixture, and rule by rule with hand-made headers."""
import io
import tarfile

import pytest

import tar_read_cases as rc
import tar_v1_reader_model as tm
import tar_writer_model as wm
from tar_open_cases import END, entry, gz, header, tarfile_image

MEMBERS = [("dir", None), ("dir/a.txt", b"alpha"), ("dir/b.bin", bytes(range(256)) * 5), ("dir/empty", b""),
           ("p" * 90 + "/" + "q" * 60 + "/r.bin", b"prefixed"), ("top", b"t" * 512)]


@pytest.mark.parametrize("wrap", [bytes, gz], ids=["plain", "gzip"])
def test_model_against_tarfile(wrap):
    """USTAR images without long names: keys, kinds, contents; mtimes of files, 0 for directories; tarfile writes the
    mode as seven digits, the model reads the first six: tarfile's mode >> 3"""
    image = tarfile_image(tarfile.USTAR_FORMAT, MEMBERS)
    data, table, counts = tm.open_stream(wrap(image))
    assert data == image
    with tarfile.open(fileobj=io.BytesIO(image)) as tf:
        infos = tf.getmembers()
        # (tarfile writes a directory's name with a trailing '/' and strips it again when it reads)
        assert list(table) == [i.name.encode() + (b"/" if i.isdir() else b"") for i in infos]
        for info, v in zip(infos, table.values()):
            assert v["kind"] == (b"5" if info.isdir() else b"0")
            assert v["contents"] == (b"" if info.isdir() else tf.extractfile(info).read())
            assert v["mtime"] == (0 if info.isdir() else info.mtime)
            assert v["mode"] == (0 if info.isdir() else info.mode >> 3)
            if not info.isdir():
                assert (v["offset"], v["size"]) == (info.offset_data, info.size)
    assert counts["headers"] == len(image) // 512 - sum((len(c or b"") + 511) // 512 for _, c in MEMBERS)
    assert counts["skipped"] == 0 and counts["nameless"] == counts["headers"] - len(MEMBERS)


@pytest.mark.parametrize("entries", rc.ROUND_TRIP + [[("a", b"A")], [("x/y", (b"", "5", 9)), ("x/y/z", (b"z" * 1024, "0", 1))]])
def test_model_reads_what_write_tarball_writes(entries):
    image = wm.image(entries)
    for img, fmt in ((image, tm.TF_DETECT), (image, tm.TF_UNCOMPRESSED), (gz(image), tm.TF_DETECT), (gz(image), tm.TF_GZIP)):
        data, table, counts = tm.open_stream(img, fmt)
        assert data == image and rc.table_rows(table) == rc.written(entries)
        assert counts == dict(headers=len(entries) + 2, nameless=2, skipped=0)


def test_model_on_the_reference_fixture():
    data, table, counts = tm.open_stream(rc.fixture())
    assert len(data) % 512 == 0
    assert (len(table), counts["headers"], counts["nameless"]) == (1743, 1750, 7)
    assert counts["skipped"] == 0 and not [k for k, v in table.items() if v["kind"] == b"5"]
    with tarfile.open(fileobj=io.BytesIO(data)) as tf:  # the independent referee: names, contents and mtimes
        infos = [i for i in tf.getmembers() if i.isfile()]
        assert [i.name.encode() for i in infos] == list(table)
        for info in infos[::97]:
            v = table[info.name.encode()]
            assert v["contents"] == tf.extractfile(info).read() and v["mtime"] == info.mtime


# ---- the rules, one hand-made header each ----
@pytest.mark.parametrize("s,value", [
    (b"00000000123", 0o123), (b"7", 7), (b"0o17", 0o17), (b"0O17", 0o17), (b"1_2_3", 0o123), (b"_1", 1), (b"1_", 1),
    (b"0o_7", 7), (b"00", 0), (b"0o0", 0), (b"77777777777", 8 ** 11 - 1),
    (b"0o", None),      # the prefix is not taken (no byte follows it): '0', then 'o' stops the scan
    (b"0o_", None), (b"0o__", None), (b"___", None), (b"", None), (b"8", None), (b"19", None), (b"1 ", None),
    (b" 1", None), (b"1\x001", None), (b"1\x00", None), (b"0x1", None), (b"o1", None), (b"0o0o1", None),
    (b"-1", None), (b"+1", None), (b"1.", None)])
def test_rule_parse_oct_int(s, value):
    if value is None:
        with pytest.raises(ValueError):
            tm.parse_oct_int(s)
    else:
        assert tm.parse_oct_int(s) == value


def test_rule_trim():
    assert tm.trim(b"ab\0cd\0") == b"ab" and tm.trim(b"\0ab") == b"" and tm.trim(b"n" * 100) == b"n" * 100
    table = tm.open_stream(entry(b"x", name=b"n" * 100, prefix=b"p" * 155) + END)[1]
    assert list(table) == [b"p" * 155 + b"/" + b"n" * 100]


def _status(image, fmt=tm.TF_DETECT):
    try:
        tm.open_stream(image, fmt)
    except tm.Stop as e:
        return e.status
    return 0


def test_rule_nameless_header_is_skipped_by_one_block():
    inner = header(name=b"in1") + header(name=b"in2")
    table, counts = tm.open_stream(header(name=b"", size=1024) + inner)[1:]
    assert list(table) == [b"in1", b"in2"] and counts == dict(headers=3, nameless=1, skipped=0)
    assert _status(header(name=b"", size_field=b"garbage!!!!\0", mtime=b"x", mode=b"y")) == 0
    assert _status(header(name=b"\0named-behind-a-nul", size_field=b"8\0")) == 0


def test_rule_numeric_slices():
    assert _status(header(name=b"n", size_field=b"0000000000 \0")) == tm.TAR_OPEN       # 11 bytes, the space inside
    assert _status(header(name=b"n", size_field=b"00000000000 ")) == 0                  # byte 12 is outside
    assert _status(header(name=b"n", mtime=b"0000000000\0\0")) == tm.TAR_OPEN
    assert _status(header(name=b"n", mode=b"00064 \0")) == tm.TAR_OPEN_MODE
    table = tm.open_stream(entry(b"", name=b"a", mode=b"0000644\0") + entry(b"", name=b"b", mode=b"100664 \0"))[1]
    assert [v["mode"] for v in table.values()] == [0o64, 0o100664]                      # the first six bytes only


def test_rule_order_inside_a_header():
    bs, bt, bm = b"0000000000 \0", b"1400000000 \0", b"00064 \0"
    assert _status(header(name=b"x", size_field=bs, mtime=bt, mode=bm)[:511]) == tm.TAR_EOF   # the whole block first
    assert _status(header(name=b"x", size_field=bs, mode=bm)) == tm.TAR_OPEN
    assert _status(header(name=b"x", mtime=bt, mode=bm)) == tm.TAR_OPEN
    assert _status(header(name=b"x", mode=bm, size=99999)) == tm.TAR_OPEN_MODE
    assert _status(header(name=b"x", size=99999)) == tm.TAR_EOF
    assert _status(header(name=b"x", size=99999, typeflag=b"Z")) == tm.TAR_EOF                # whatever the type


def test_rule_prefix_needs_the_six_bytes():
    def key(magic):
        return list(tm.open_stream(entry(b"", name=b"n", prefix=b"p", magic=magic))[1])[0]
    assert key(b"ustar\0" + b"00") == b"p/n" and key(b"ustar\0") == b"p/n"
    assert key(b"ustar  \0") == b"n" and key(b"ustarx") == b"n" and key(b"") == b"n" and key(b"USTAR\0") == b"n"


def test_rule_join_and_to_unix_path():
    def key(prefix, name):
        return list(tm.open_stream(entry(b"", name=name, prefix=prefix))[1])[0]
    assert [key(p, n) for p, n in [(b"pre", b"name"), (b"pre/", b"name"), (b"pre", b"/name"), (b"pre/", b"/name")]] == [b"pre/name"] * 4
    assert key(b"", b"name") == b"name" and key(b"", b"/abs") == b"/abs"  # no path check at open
    assert key(b"a\\b", b"c\\d") == b"a/b/c/d" and key(b"", b"..\\..\\up") == b"../../up"
    assert key(b"a\\", b"b") == b"a//b"  # the join sees the backslash: it adds its '/', toUnixPath comes after


def test_rule_type_flags_and_the_table():
    img = b"".join(entry(b"data%d" % i, name=b"k%d" % i, typeflag=t) for i, t in enumerate(
        [b"0", b"\0", b"5", b"1", b"2", b"L", b"x", b"g", b"Z", b"\xff"]))
    table, counts = tm.open_stream(img)[1:]
    assert [(k, v["kind"]) for k, v in table.items()] == [(b"k0", b"0"), (b"k1", b"0"), (b"k2", b"5")]
    assert counts["skipped"] == 7
    assert table[b"k2"] == dict(kind=b"5", contents=b"", mtime=0, mode=0, offset=0, size=0)
    assert table[b"k1"]["contents"] == b"data1" and table[b"k1"]["offset"] == 3 * 512
    # a repeated key: the earlier place, the later value; \ and / are one key
    img = entry(b"1", name=b"a\\b") + entry(b"2", name=b"c") + entry(b"3", name=b"a/b", typeflag=b"5") + entry(b"4", name=b"c")
    table = tm.open_stream(img)[1]
    assert [(k, v["kind"], v["contents"]) for k, v in table.items()] == [(b"a/b", b"5", b""), (b"c", b"0", b"4")]


def test_rule_position_and_end():
    assert _status(header(name=b"five", size=5) + b"12345") == 0               # unpadded last entry
    assert _status(header(name=b"six", size=6) + b"12345") == tm.TAR_EOF
    assert _status(header(name=b"a", size=700) + bytes(700) + b"x") == 0       # the padded end passes the image
    assert _status(header(name=b"a") + b"x") == tm.TAR_EOF
    assert _status(b"", tm.TF_UNCOMPRESSED) == 0 and tm.open_stream(bytes(1024))[1] == {}


def test_rule_format():
    good = entry(b"ok", name=b"ok") + END
    assert _status(b"\x1f\0" + good[2:]) == tm.TAR_FORMAT and _status(b"\x1f\0" + good[2:], tm.TF_UNCOMPRESSED) == 0
    assert _status(b"") == tm.TAR_FORMAT and _status(b"\x1f") == tm.TAR_FORMAT and _status(b"a") == tm.TAR_EOF
    assert _status(gz(good)) == 0 and _status(gz(b"")) == 0
    assert _status(good, tm.TF_GZIP) is None and _status(gz(good)[:17]) is None  # the decoder's
    g = bytearray(gz(good))
    g[-1] ^= 1  # a wrong ISIZE is an error here: dfGzip, not trustSize
    assert _status(bytes(g)) is None
    assert _status(gz(good), tm.TF_UNCOMPRESSED) == tm.TAR_EOF


def test_cases_are_built_for_what_the_model_says():
    for name, image, fmt, want in rc.all_cases():
        assert rc.built_for(tm.expected(image, fmt)[0], want), name
