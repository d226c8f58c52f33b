"""CPU-only: zh_zip_create_batch (zippy_amd/csrc/zh_zip_write.hip, zh_zip_create_kernel) under the fiber emulator of
tests/hipemu, with the emulator's 128 KiB staging chunks, so that entries cross chunk borders.  The device's archives
must equal oracle.zip_oracle.create_archive byte for byte; at levels other than BestSpeed, the same framing around the
oracle's streams of that level (tests/zip_v2_writer_model.py)."""
import ctypes as c
import io
import zipfile

import pytest

import emu
import synth
import zip_v2_writer_model as zm
from oracle import zip_oracle
from zippy_amd.common import ZippyError

T, D = 0x6000, 0x5521


@pytest.fixture(scope="module")
def eng():
    return emu.engine()


def _blob(n, seed=1):
    return bytes((i * 131 + seed * 7 + (i >> 7) + (i * i >> 11)) & 0xFF for i in range(n))


SIZES = [0, 1, 3, 4, 15, 16, 17, 140000]


def _sized(prefix="f"):
    return [("%s%d.bin" % (prefix, n), _blob(n, n)) for n in SIZES]


ENTRY_SETS = [
    _sized(),
    [("one.txt", b"hello")],
    [("dir/", b""), ("dir/a", _blob(1000, 3)), ("ünicøde/日本語.txt", "UTF-8".encode() * 40), ("a//b", b"zzz")],
    [("x" * 300, _blob(3000, 5)), ("y" * 65535, b"long"), ("z", b"")],
    [],
]


def test_model_is_the_oracle_at_best_speed():
    """the helper the level tests rest on restates create_archive: equal at the reference's level"""
    for entries in ENTRY_SETS:
        assert zm.image(entries, T, D) == zip_oracle.create_archive(entries, T, D)
    assert zm.image([]) == zip_oracle.create_archive([]) and len(zm.image([])) == 98
    stamped = [("a", (b"one", 1, 2)), ("b", (b"", 3, 4))]
    assert zm.image(stamped)[10:14] == bytes([3, 0, 4, 0])  # "b" goes first, with its own pair
    assert zm.framing(zm.image(ENTRY_SETS[0], T, D))[0] == zm.framing(zm.image(ENTRY_SETS[0], T, D, 9))[0]


def test_emu_zipc_entry_sizes(eng):
    entries = _sized()
    img = eng.create_zips_one(entries, T, D)
    assert img == zip_oracle.create_archive(entries, T, D)
    with zipfile.ZipFile(io.BytesIO(img)) as zf:
        assert zf.testzip() is None
        assert zf.namelist() == [p for p, _ in reversed(entries)]  # listed last to first
        assert [zf.read(p) for p, _ in entries] == [v for _, v in entries]


def test_emu_zipc_stream_alignments(eng):
    """path lengths chosen so that the streams start at every residue mod 16 (the 20-byte extra sits between the path
    and the stream), the local headers and the central directory records with them"""
    import oracle
    proc, starts, o = [], [], 0  # in processing order
    for i in range(32):
        contents = _blob(40 + 97 * i, i)
        plen = (i - o - 50) % 16 + 16
        proc.append((("n%d_" % i).ljust(plen, "x"), contents))
        starts.append(o + 30 + plen + 20)
        o += 30 + plen + 20 + len(oracle.compress(contents, 1, oracle.dfDeflate))
    assert {s % 16 for s in starts} == set(range(16))
    entries = proc[::-1]
    img = eng.create_zips_one(entries, T, D)
    assert img == zip_oracle.create_archive(entries, T, D)
    for (p, v), at in zip(proc, starts):
        assert img[at - 20 - len(p):at - 20] == p.encode()
        assert img[at:at + 9] == oracle.compress(v, 1, oracle.dfDeflate)[:9]


def test_emu_zipc_record_alignments(eng):
    """one call of 32 archives whose central directories and end records start at every residue mod 16, the odd ones
    too (records are 124 bytes and two paths an entry: only a stream of odd length moves the end records to an odd
    place)"""
    tables = [[("p" * plen, _blob(n, n))] for plen in range(1, 17) for n in (10, 11)]
    want = [zip_oracle.create_archive(t, T, D) for t in tables]
    cd = {int.from_bytes(w[-98 + 48:-98 + 56], "little") % 16 for w in want}
    end = {(len(w) - 98) % 16 for w in want}
    assert cd == end == set(range(16))
    outs, sts = eng.create_zips(tables, T, D)
    assert sts == [0] * 32 and outs == want


@pytest.mark.parametrize("level", [-2, 0, 1, -1, 9])
def test_emu_zipc_levels(eng, level):
    entries = _sized()[:7] + [("text/alice.txt", synth.corpus_file("alice29.txt")[:60000])]
    img = eng.create_zips_one(entries, T, D, level)
    assert img == zm.image(entries, T, D, level)
    with zipfile.ZipFile(io.BytesIO(img)) as zf:
        assert zf.testzip() is None


def test_emu_zipc_per_entry_times(eng):
    entries = [("a", (b"one", 1, 2)), ("b", (b"", 3, 4)), ("c", b"call's pair")]
    assert eng.create_zips_one(entries, T, D) == zm.image(entries, T, D)


def test_emu_zipc_empty_table(eng):
    outs, sts = eng.create_zips([[], [("a", b"x")], {}])
    assert sts == [0, 0, 0]
    assert outs[0] == outs[2] == zip_oracle.create_archive([]) and len(outs[0]) == 98
    assert outs[1] == zip_oracle.create_archive([("a", b"x")])
    with zipfile.ZipFile(io.BytesIO(outs[0])) as zf:
        assert zf.namelist() == []
    assert eng.create_zips([]) == ([], [])


@pytest.mark.parametrize("k", range(len(ENTRY_SETS)))
def test_emu_zipc_batch_of_one_equals_zh_zip_create(eng, k):
    entries = ENTRY_SETS[k]
    outs, sts = eng.create_zips([entries], T, D)
    assert sts == [0] and outs[0] == eng.create_zip(entries, T, D)


def _raw_create(eng, table):
    """zh_zip_create through ctypes; contents None: a NULL pointer with the length given -> (rc, archive or None)"""
    n = len(table)
    names = (c.c_char_p * n)(*[p for p, _, _ in table])
    nlens = (c.c_size_t * n)(*[len(p) for p, _, _ in table])
    blobs = (c.c_void_p * n)(*[c.cast(c.c_char_p(b), c.c_void_p) if b else None for _, b, _ in table])
    blens = (c.c_size_t * n)(*[ln for _, _, ln in table])
    dst, dlen = c.c_void_p(0xDEAD000), c.c_size_t(12345)
    rc = eng.lib.zh_zip_create(eng._h, names if n else None, nlens if n else None, blobs if n else None,
                               blens if n else None, n, T, D, c.byref(dst), c.byref(dlen))
    try:
        return rc, c.string_at(dst, dlen.value) if dst.value else None
    finally:
        eng.lib.zh_free(dst)


def test_emu_zip_create_precedence(eng):
    """zh_zip_create's own checks run last to first and the entry processed first decides: a missing path reads
    ZH_ERR_ZIP_NAME, missing contents ZH_ERR_ARGUMENT (zh_zip_create_batch's call-level checks would say otherwise);
    no entries with NULL arrays: the 98 bytes"""
    assert _raw_create(eng, [(b"ok", None, 5), (b"", b"x", 1)]) == (zm.ZH_ERR_ZIP_NAME, None)
    assert _raw_create(eng, [(b"", b"x", 1), (b"ok", None, 5)]) == (zm.ZH_ERR_ARGUMENT, None)
    assert _raw_create(eng, [(b"a", b"1", 1), (b"a", b"2", 1)]) == (zm.ZH_ERR_ZIP_DUPLICATE, None)
    assert _raw_create(eng, []) == (0, zm.image([], T, D))
    assert len(zm.image([], T, D)) == 98


def test_emu_zipc_whole_batch_equals_one_by_one(eng):
    outs, sts = eng.create_zips(ENTRY_SETS, T, D)
    assert sts == [0] * len(ENTRY_SETS)
    assert outs == [eng.create_zip(e, T, D) for e in ENTRY_SETS] == [zip_oracle.create_archive(e, T, D) for e in ENTRY_SETS]


@pytest.mark.parametrize("entries,status", [
    ([("ok", b"1"), ("", b"x")], zm.ZH_ERR_ZIP_NAME),
    ([("/abs/path.txt", b"x"), ("ok", b"1")], zm.ZH_ERR_ZIP_NAME),
    ([("x" * 65536, b"")], zm.ZH_ERR_ZIP_NAME),
    ([("a", b"1"), ("b", b"2"), ("a", b"")], zm.ZH_ERR_ZIP_DUPLICATE),
    # two faults each: the checks run last to first, so the fault nearer the END of the table wins
    ([("a", b""), ("a", b"1"), ("", b"x")], zm.ZH_ERR_ZIP_NAME),
    ([("/abs", b""), ("b", b"1"), ("b", b"2")], zm.ZH_ERR_ZIP_DUPLICATE),
])
def test_emu_zipc_errors(eng, entries, status):
    assert zm.status(entries) == status
    outs, sts = eng.create_zips([entries], T, D)
    assert outs == [None] and sts == [status]
    with pytest.raises(ZippyError) as ei:
        eng.create_zips_one(entries, T, D)
    assert ei.value.status == status
    with pytest.raises(ZippyError) as ej:  # zh_zip_create agrees
        eng.create_zip(entries, T, D)
    assert ej.value.status == status
    assert eng.lib.zh_strerror(status).decode().startswith(
        {33: "Invalid file name", 31: "Unsupported archive, duplicate entry"}[status])


def test_emu_zipc_batch_mixes_good_and_bad(eng):
    good = [e for e in ENTRY_SETS]
    bad = [[("", b"x")], [("a", b""), ("a", b"")], [("/abs", b"x")], [("x" * 65536, b"y"), ("fine", b"z")]]
    zips = [good[0], bad[0], good[1], bad[1], good[2], bad[2], good[3], bad[3], good[4]]
    want = [zm.status(z) for z in zips]
    assert sorted(set(want)) == [0, zm.ZH_ERR_ZIP_DUPLICATE, zm.ZH_ERR_ZIP_NAME]
    outs, sts = eng.create_zips(zips, T, D)
    assert sts == want
    for z, out, st in zip(zips, outs, sts):
        assert out == (zip_oracle.create_archive(z, T, D) if st == 0 else None)
    alone, sts = eng.create_zips(good, T, D)  # the good ones alone: the same bytes
    assert sts == [0] * len(good) and alone == [o for o in outs if o is not None]


def test_emu_zipc_call_level_errors(eng):
    with pytest.raises(ZippyError) as ei:
        eng.create_zips([[("a", b"x")]], T, D, 10)
    assert ei.value.status == 1  # ZH_ERR_INVALID_LEVEL


def _raw_call(eng, entries, first, level):
    """zh_zip_create_batch through ctypes with a hand-made table, poisoned outputs -> (rc, dsts, dst_lens, statuses)"""
    from zippy_amd._binding import ZipNewEntry
    n = len(first) - 1
    arr = None if entries is None else (ZipNewEntry * len(entries))(*entries)
    dsts = (c.c_void_p * n)(*[0xDEAD000 + 16 * t for t in range(n)])
    dlens, sts = (c.c_size_t * n)(*[12345] * n), (c.c_int32 * n)(*[77] * n)
    rc = eng.lib.zh_zip_create_batch(eng._h, arr, (c.c_size_t * len(first))(*first), n, level, dsts, dlens, sts)
    return rc, list(dsts), list(dlens), list(sts)


def _entry(path, contents, path_len=None, length=None):
    """a ZipNewEntry with the pointers as given (None: NULL) and the lengths of the data unless given"""
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
def test_emu_zipc_c_level_refusals(eng, table, first, level, rc):
    entries = None if table is None else [_entry(*e) for e in table]
    n = len(first) - 1
    assert _raw_call(eng, entries, first, level) == (rc, [None] * n, [0] * n, [0] * n)


def test_emu_zipc_is_directory_is_not_read(eng):
    """the raw table with is_directory set and a NULL path of length 0: external attributes stay 0, and the empty
    path is the archive's own ZH_ERR_ZIP_NAME, not a call-level error"""
    e = _entry(b"d/", b"")
    e.is_directory, e.dos_time, e.dos_date = 1, T, D
    rc, dsts, dlens, sts = _raw_call(eng, [e, _entry(None, None)], [0, 1, 2], 1)
    assert (rc, sts, dsts[1], dlens[1]) == (0, [0, zm.ZH_ERR_ZIP_NAME], None, 0)
    try:
        assert c.string_at(dsts[0], dlens[0]) == zip_oracle.create_archive([("d/", b"")], T, D)
    finally:
        eng.lib.zh_free(dsts[0])


def test_emu_zipc_first_cap_retry(eng, monkeypatch):
    """ZH_COMPRESS_FIRST_CAP=64: the larger contents of a mixed batch outgrow their first slots and are compressed again
    into zh_compress_bound slots (their CRC-32s with them) -- the same bytes as without it, the oracle's"""
    zips = [_sized(), [], [("d/", b""), ("d/x", _blob(1000, 3))], [("", b"bad")],
            [("t.txt", synth.corpus_file("alice29.txt")[:30000])]]
    want = eng.create_zips(zips, T, D)
    monkeypatch.setenv("ZH_COMPRESS_FIRST_CAP", "64")
    assert eng.create_zips(zips, T, D) == want
    assert want == ([None if zm.status(z) else zip_oracle.create_archive(z, T, D) for z in zips],
                    [zm.status(z) for z in zips])


def test_emu_zipc_round_trip_zh_zip_open(eng):
    entries = [("r/%d" % i, _blob(37 * i, i)) for i in range(1, 40)] + [("r/", b"")]
    img = eng.create_zips_one(entries, T, D)
    reader = eng.open_zip(img)
    assert [e["path"] for e in reader.entries] == [p for p, _ in reversed(entries)]
    files = [i for i, e in enumerate(reader.entries) if not e["is_directory"]]
    outs, sts = reader.extract_batch(files)
    assert sts == [0] * 39 and outs == [v for _, v in reversed(entries[:39])]
    reader.close()


def test_emu_zipc_mmap_contents(eng):
    """contents given as a writable buffer go to the library without a copy"""
    import mmap
    from zippy_amd._binding import _buffer_address
    mm = mmap.mmap(-1, 5000)
    mm[:] = _blob(5000, 9)
    try:
        prep = eng.prepare_zips_v2([[("m", mm)]], T, D)
        assert prep[0][0].contents == _buffer_address(mm)[0] and prep[0][0].len == 5000  # the mapping's own address
        outs, sts = eng.create_zips_prepared(prep)
        assert sts == [0] and outs[0] == zip_oracle.create_archive([("m", bytes(mm))], T, D)
        del prep
    finally:
        import gc
        gc.collect()
        mm.close()
