"""CPU-only: zh_zip_write_batch (zippy_amd/csrc/zh_zip_write.hip) under the fiber emulator of tests/hipemu, with the
emulator's 128 KiB staging chunks, so that entries cross chunk borders.  The device's archives must equal
tests/zip_v1_writer_model.py byte for byte."""
import io
import os
import zipfile

import pytest

import emu
import synth
import zip_v1_writer_model as zm
import zip_write_cases
from zip_write_cases import SIZES, blob as _blob
from zippy_amd.common import ZippyError


@pytest.fixture(scope="module")
def eng():
    return emu.engine()


def test_emu_zip_entry_sizes(eng):
    entries = [("f%d.bin" % n, (_blob(n, n), False, 0x6000 + i, 0x5521)) for i, n in enumerate(SIZES)]
    assert eng.write_zip(entries) == zm.image(entries)


def test_emu_zip_record_alignments(eng):
    """path lengths chosen so that entry i's stream starts at i mod 16: the streams go to every alignment, and the
    records behind them (local headers, central directory records, the end record) with them"""
    import oracle
    entries, starts, o = [], [], 0
    for i in range(32):
        contents = _blob(40 + 97 * i, i)
        plen = (i - o - 30) % 16 + 16
        entries.append((("n%d_" % i).ljust(plen, "x"), (contents, False, i, i)))
        starts.append(o + 30 + plen)
        o += 30 + plen + len(oracle.compress(contents, -1, oracle.dfDeflate))
        entries.append(("ef"[i // 16] * (i % 16 + 1) + "/", (b"", True, i, i)))
        o += 30 + i % 16 + 2
    assert {s % 16 for s in starts} == set(range(16))
    img = eng.write_zip(entries)
    assert img == zm.image(entries)
    assert all(img[at - len(p):at] == p.encode() for (p, _), at in zip(entries[::2], starts))


def test_emu_zip_end_record_alignments(eng):
    zip_write_cases.check_end_record_alignments(eng)


def test_emu_zip_directories_and_paths(eng):
    entries = [("dir/", (b"", True, 1, 2)), ("dir2", (b"contents of a directory", True, 3, 4)),
               ("/abs/path.txt", b"absolute"), ("ünicøde/日本語.txt", "UTF-8".encode() * 40), ("", b""),
               ("a//b", b"zzz"), ("x" * 300, _blob(3000, 5))]
    img = eng.write_zip(entries)
    assert img == zm.image(entries)
    with zipfile.ZipFile(io.BytesIO(img)) as zf:
        assert zf.testzip() is None
        assert [i.external_attr for i in zf.infolist()][:2] == [0x10, 0x10]


@pytest.mark.parametrize("level", [-2, 0, 1, -1, 9])
def test_emu_zip_levels(eng, level):
    entries = [("f%d" % n, _blob(n, n)) for n in SIZES[:7]] + [
        ("text/alice.txt", (synth.corpus_file("alice29.txt")[:60000], False, 0x6000, 0x5521))]
    assert eng.write_zip(entries, level) == zm.image(entries, level)


@pytest.mark.parametrize("entries,status", [
    ([], zm.ZH_ERR_ZIP_EMPTY),
    ([("x" * 65536, b"")], zm.ZH_ERR_ZIP_TOO_LARGE),
    ([("d/", b"x")], zm.ZH_ERR_ARGUMENT),
    ([("", b"x")], zm.ZH_ERR_ARGUMENT),
    ([("a", b"1"), ("b", b"2"), ("a", b"")], zm.ZH_ERR_ZIP_DUPLICATE),
    ([("a", b""), ("a", b""), ("d/", b"x"), ("x" * 65536, b"")], zm.ZH_ERR_ZIP_TOO_LARGE),
    ([("a", b""), ("a", b""), ("d/", b"x")], zm.ZH_ERR_ARGUMENT),
])
def test_emu_zip_errors(eng, entries, status):
    assert zm.status(entries) == status
    outs, sts = eng.write_zips([entries])
    assert outs == [None] and sts == [status]
    with pytest.raises(ZippyError) as ei:
        eng.write_zip(entries)
    assert ei.value.status == status
    assert eng.lib.zh_strerror(status).decode().startswith(
        {40: "Zip archive has no contents", 41: "Zip archive too large", 22: "Invalid argument",
         31: "Unsupported archive, duplicate entry"}[status][:20])


def test_emu_zip_call_level_errors(eng):
    with pytest.raises(ZippyError) as ei:
        eng.write_zips([[("a", b"x")]], 10)
    assert ei.value.status == 1  # ZH_ERR_INVALID_LEVEL
    assert eng.write_zips([]) == ([], [])


def _raw_zip_call(eng, entries, first, level):
    """zh_zip_write_batch through ctypes with a hand-made table, poisoned outputs -> (rc, dsts, dst_lens, statuses)"""
    import ctypes as c
    from zippy_amd._binding import ZipNewEntry
    n = len(first) - 1
    arr = None if entries is None else (ZipNewEntry * len(entries))(*entries)
    dsts = (c.c_void_p * n)(*[0xDEAD000 + 16 * t for t in range(n)])
    dlens, sts = (c.c_size_t * n)(*[12345] * n), (c.c_int32 * n)(*[77] * n)
    rc = eng.lib.zh_zip_write_batch(eng._h, arr, (c.c_size_t * len(first))(*first), n, level, dsts, dlens, sts)
    return rc, list(dsts), list(dlens), list(sts)


def _zip_entry(path, contents, path_len=None, length=None):
    """a ZipNewEntry with the pointers as given (None: NULL) and the lengths of the data unless given"""
    import ctypes as c
    from zippy_amd._binding import ZipNewEntry
    return ZipNewEntry(path, len(path or b"") if path_len is None else path_len,
                       c.cast(c.c_char_p(contents), c.c_void_p) if contents else None,
                       len(contents or b"") if length is None else length, 0, 0, 0)


_GOOD = [(b"a", b"xy"), (b"b", b"z")]


@pytest.mark.parametrize("table,first,level,rc", [
    (_GOOD, [0, 2, 1], 1, zm.ZH_ERR_ARGUMENT),  # decreasing first[]
    (None, [0, 0, 1], 1, zm.ZH_ERR_ARGUMENT),  # entries == NULL with a non-zero count
    ([(b"a", b"xy"), (None, b"z", 1)], [0, 1, 2], 1, zm.ZH_ERR_ARGUMENT),  # path NULL, path_len 1
    ([(b"a", b"xy"), (b"b", None, None, 5)], [0, 1, 2], -1, zm.ZH_ERR_ARGUMENT),  # contents NULL, len 5
    (_GOOD, [0, 2, 1], 10, 1),  # the level is checked before the table (ZH_ERR_INVALID_LEVEL)
    (None, [0, 1], -3, 1),
])
def test_emu_zip_c_level_refusals(eng, table, first, level, rc):
    entries = None if table is None else [_zip_entry(*e) for e in table]
    n = len(first) - 1
    assert _raw_zip_call(eng, entries, first, level) == (rc, [None] * n, [0] * n, [0] * n)


def test_emu_zip_batch_mixes_good_and_bad(eng):
    good = [[("one.txt", b"hello")],
            [("f%d" % n, _blob(n, n)) for n in SIZES],
            [("d/", (b"", True, 1, 1)), ("d/x", _blob(1000, 3))],
            [("only/", (b"", True, 0, 0))]]
    bad = [[], [("d/", b"x")], [("a", b""), ("a", b"")]]
    zips = [good[0], bad[0], good[1], bad[1], good[2], bad[2], good[3]]
    want = [zm.status(z) for z in zips]
    assert sorted(set(want)) == [0, zm.ZH_ERR_ARGUMENT, zm.ZH_ERR_ZIP_DUPLICATE, zm.ZH_ERR_ZIP_EMPTY]
    outs, sts = eng.write_zips(zips)
    assert sts == want
    for z, out, st in zip(zips, outs, sts):
        assert out == (zm.image(z) if st == 0 else None)
    # the good ones alone: the same bytes
    alone, sts = eng.write_zips(good)
    assert sts == [0] * 4 and alone == [o for o in outs if o is not None]


def test_emu_zip_first_cap_retry(eng, monkeypatch):
    """ZH_COMPRESS_FIRST_CAP=64: the larger contents of a mixed batch outgrow their first slots and are compressed again
    into zh_compress_bound slots (their CRC-32s with them) -- the same bytes as without it, the model's"""
    zips = [[("f%d" % n, _blob(n, n)) for n in SIZES], [], [("d/", (b"", True, 1, 1)), ("d/x", _blob(1000, 3))],
            [("only/", (b"", True, 0, 0))], [("t.txt", synth.corpus_file("alice29.txt")[:30000])]]
    want = eng.write_zips(zips)
    monkeypatch.setenv("ZH_COMPRESS_FIRST_CAP", "64")
    assert eng.write_zips(zips) == want
    assert want == ([zm.image(z) if z else None for z in zips], [zm.status(z) for z in zips])


def test_emu_zip_post_compression_refusal(eng, monkeypatch):
    """step 5 through ZH_ZIP32_LIMIT (read at each call): the compressed length, a local header's offset, the
    central directory's offset -- the other archives of the call keep their bytes"""
    big = [("a", _blob(3000, 1)), ("b", _blob(500, 2))]
    small = [("s", b"small")]
    img = zm.image(big)
    cd_off = int.from_bytes(img[-6:-2], "little")
    clen_a = int.from_bytes(img[18:22], "little")
    for limit in (clen_a, cd_off, cd_off + 1):
        want = zm.status(big, limit=limit)
        monkeypatch.setenv("ZH_ZIP32_LIMIT", str(limit))
        outs, sts = eng.write_zips([small, big, small])
        assert sts == [0, want, 0]
        assert outs[0] == outs[2] == zm.image(small)
        assert outs[1] == (img if want == 0 else None)
    assert [zm.status(big, limit=x) for x in (clen_a, cd_off, cd_off + 1)] == [41, 41, 0]
    monkeypatch.delenv("ZH_ZIP32_LIMIT")
    assert eng.write_zip(big) == img


def test_emu_zip_round_trip_zh_zip_open(eng):
    entries = [("r/%d" % i, (_blob(37 * i, i), False, i, i)) for i in range(1, 40)] + [("r/", (b"", True, 0, 0))]
    img = eng.write_zip(entries)
    reader = eng.open_zip(img)
    assert [e["path"] for e in reader.entries] == [p for p, _ in entries]
    outs, sts = reader.extract_batch(list(range(39)))
    assert sts == [0] * 39 and outs == [v[0] for _, v in entries[:39]]
    reader.close()


def test_emu_zip_mmap_contents(eng):
    """contents given as a writable buffer go to the library without a copy"""
    import mmap
    mm = mmap.mmap(-1, 5000)
    mm[:] = _blob(5000, 9)
    try:
        assert eng.write_zip([("m", mm)]) == zm.image([("m", bytes(mm))])
    finally:
        import gc
        gc.collect()
        mm.close()
    assert os.environ.get("ZH_ZIP32_LIMIT") is None
