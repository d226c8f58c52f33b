"""CPU checks of tests/zip_v1_writer_model.py, the restatement of writeZipArchive (ziparchives_v1.nim:371-486) that
the device tests compare against: one small archive pinned byte for byte, archives read back by Python's zipfile, by
the restatement of the reference's reader (oracle/zip_oracle.py) and by zh_zip_open (under the fiber emulator), the
splitFile rule and every status in its order of precedence."""
import io
import zipfile

import pytest

import zip_v1_writer_model as zm


def h(s):
    return bytes.fromhex(s.replace(" ", ""))


# writeZipArchive of [("d/", ekDirectory), ("e", ekFile ""), ("h.txt", ekFile "Hello, World!")], every entry with
# toMsDos = (0x6000 12:00:00, 0x5521 2022-09-01), worked out from ziparchives_v1.nim:379-477 field by field
T, D = "0060", "2155"  # 0x6000, 0x5521 little-endian
PINNED = (
    # local header of "d/" at 0: sig, version 20, flags 0x0800, method 0, time, date, crc 0, lengths 0, name 2, extra 0
    h("504b0304 1400 0008 0000" + T + D + "00000000 00000000 00000000 0200 0000") + b"d/"
    # "e" at 32: empty contents, method 0
    + h("504b0304 1400 0008 0000" + T + D + "00000000 00000000 00000000 0100 0000") + b"e"
    # "h.txt" at 63: method 8, crc32 0xec4ac3d0, compressed 18, length 13
    + h("504b0304 1400 0008 0800" + T + D + "d0c34aec 12000000 0d000000 0500 0000") + b"h.txt"
    # compress("Hello, World!", DefaultCompression, dfDeflate): one stored block (final, LEN 13, NLEN ~13)
    + h("01 0d00 f2ff") + b"Hello, World!"
    # central directory at 116: sig, made-by 63, version 20, flags, method, time, date, crc, lengths, name length,
    # extra / comment / disk / internal 0, external attributes (0x10 directory, 0x20 file), local header offset
    + h("504b0102 3f00 1400 0008 0000" + T + D + "00000000 00000000 00000000 0200 0000 0000 0000 0000"
        "10000000 00000000") + b"d/"
    + h("504b0102 3f00 1400 0008 0000" + T + D + "00000000 00000000 00000000 0100 0000 0000 0000 0000"
        "20000000 20000000") + b"e"
    + h("504b0102 3f00 1400 0008 0800" + T + D + "d0c34aec 12000000 0d000000 0500 0000 0000 0000 0000"
        "20000000 3f000000") + b"h.txt"
    # end of central directory at 262: 3 entries twice, size 146, offset 116, comment length 0
    + h("504b0506 0000 0000 0300 0300 92000000 74000000 0000"))


def _pinned_entries():
    return [("d/", (b"", True, 0x6000, 0x5521)), ("e", (b"", False, 0x6000, 0x5521)),
            ("h.txt", (b"Hello, World!", False, 0x6000, 0x5521))]


def test_pinned_archive():
    assert len(PINNED) == 284
    assert zm.image(_pinned_entries()) == PINNED


@pytest.mark.parametrize("path,name", [
    (b"", b""), (b"/", b""), (b"a/", b""), (b"a/b/", b""), (b"d", b"d"), (b"a/b.txt", b"b"), (b"/abs/x.tar.gz", b"x.tar"),
    (b".bashrc", b".bashrc"), (b"a/.bashrc", b".bashrc"), (b"a..", b"a.."), (b"a.b.", b"a"), (b".", b"."),
    (b"..", b".."), (b"a/..", b".."), (b"x.", b"x."), (b"a/b.c/d", b"d"), ("été.txt".encode(), "été".encode()),
])
def test_split_file_name(path, name):
    """std/os splitFile(path).name (POSIX): the rule the writer keeps is that it is empty exactly when the path is
    empty or ends in '/'"""
    assert zm.split_file_name(path) == name
    assert zm.stored(path) == (path == b"" or path.endswith(b"/"))


def _sample():
    return [("README.txt", (b"Hello, World!" * 20, False, 0x6000, 0x5521)),
            ("docs/", (b"", True, 0x6001, 0x5522)),
            ("docs/guide.md", b"# guide\n" * 300),
            ("docs/empty", b""),
            ("data/" + "d" * 140 + "/blob.bin", (bytes(range(256)) * 9, False, 7, 0x21)),
            ("ünicøde/日本.txt", "UTF-8 names".encode() * 5),
            ("bin/tiny", b"x")]


def test_image_reads_back_with_zipfile():
    entries = _sample()
    img = zm.image(entries)
    with zipfile.ZipFile(io.BytesIO(img)) as zf:
        assert zf.testzip() is None
        infos = zf.infolist()
        assert [i.filename for i in infos] == [p for p, _ in entries]
        for info, (p, v) in zip(infos, entries):
            contents, is_dir, t, d = v + (False, 0, 0)[len(v) - 1:] if isinstance(v, tuple) else (v, False, 0, 0)
            assert info.is_dir() == p.endswith("/")
            assert info.external_attr == (0x10 if is_dir else 0x20) and info.create_version == 63
            assert info.flag_bits == 0x800 and info.compress_type == (8 if contents else 0)
            assert info.date_time == ((d >> 9) + 1980, (d >> 5) & 15, d & 31, t >> 11, (t >> 5) & 63, (t & 31) * 2)
            if not info.is_dir():
                assert zf.read(info) == contents


def _expected(entries):
    return [(p.encode(), v[0] if isinstance(v, tuple) else v) for p, v in entries]


def test_image_reads_back_with_the_reference_reader():
    from oracle import zip_oracle
    entries = _sample()
    r = zip_oracle.open_archive(zm.image(entries))
    assert list(r.records) == [p for p, _ in _expected(entries)]
    for p, contents in _expected(entries):
        if p.endswith(b"/"):
            assert r.records[p]["is_directory"]
        else:
            assert zip_oracle.extract_file(r, p) == contents


def test_image_reads_back_with_zh_zip_open():
    import emu
    eng = emu.engine()
    entries = _sample()
    reader = eng.open_zip(zm.image(entries))
    assert [e["path"].encode() for e in reader.entries] == [p for p, _ in _expected(entries)]
    idx = [i for i, e in enumerate(reader.entries) if not e["is_directory"]]
    outs, sts = reader.extract_batch(idx)
    assert sts == [0] * len(idx)
    assert outs == [c for p, c in _expected(entries) if not p.endswith(b"/")]
    reader.close()


def test_model_statuses():
    ok = [("a", b"1")]
    assert zm.status(ok) == 0
    assert zm.status([]) == zm.ZH_ERR_ZIP_EMPTY
    # step 2: sizes and counts
    assert zm.status([("p%d" % i, b"") for i in range(65535)]) == 0
    assert zm.status([("p%d" % i, b"") for i in range(65536)]) == zm.ZH_ERR_ZIP_TOO_LARGE
    assert zm.status([("x" * 65535, b"")]) == 0
    assert zm.status([("x" * 65536, b"")]) == zm.ZH_ERR_ZIP_TOO_LARGE
    # step 3: contents under a path whose splitFile name is empty
    assert zm.status([("dir/", b"")]) == 0 and zm.status([("", b"")]) == 0
    assert zm.status([("dir/", b"x")]) == zm.ZH_ERR_ARGUMENT
    assert zm.status([("", b"x")]) == zm.ZH_ERR_ARGUMENT
    assert zm.status([("dir/", (b"x", True, 0, 0))]) == zm.ZH_ERR_ARGUMENT
    assert zm.status([("/abs/file", b"x")]) == 0  # v1 writes absolute paths as given
    # step 4: a repeated key
    assert zm.status([("a", b"1"), ("b", b"2"), ("a", b"")]) == zm.ZH_ERR_ZIP_DUPLICATE
    # precedence: 2 before 3 before 4, whatever the order of the entries
    assert zm.status([("a", b""), ("a", b""), ("d/", b"x"), ("x" * 65536, b"")]) == zm.ZH_ERR_ZIP_TOO_LARGE
    assert zm.status([("a", b""), ("a", b""), ("d/", b"x")]) == zm.ZH_ERR_ARGUMENT
    # step 5: after compression (a lowered limit stands for 2^32)
    big = [("a", bytes(range(256)) * 4), ("b", b"y" * 100)]
    img = zm.image(big)
    cd_off = int.from_bytes(img[-6:-2], "little")
    cd_size = int.from_bytes(img[-10:-6], "little")
    clen_a = int.from_bytes(img[18:22], "little")
    assert zm.status(big, limit=len(img)) == 0
    assert zm.status(big, limit=clen_a) == zm.ZH_ERR_ZIP_TOO_LARGE                # a compressed length
    assert zm.status(big, limit=max(clen_a, cd_size) + 1) == zm.ZH_ERR_ZIP_TOO_LARGE  # b's offset / the cd offset
    assert zm.status(big, limit=cd_off + 1) == 0
    assert zm.status(big, limit=cd_off) == zm.ZH_ERR_ZIP_TOO_LARGE
    # ... and steps 1-4 go first
    assert zm.status([("d/", b"x")] + big, limit=1) == zm.ZH_ERR_ARGUMENT
