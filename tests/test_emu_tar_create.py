"""CPU-only: zh_tar_create_batch (zippy_amd/csrc/zh_tar_create.hip) under the fiber emulator of tests/hipemu, with
the emulator's 128 KiB staging chunks, so that entries cross chunk borders.  The device's images must equal
tests/tar_writer_model.py byte for byte, its .tar.gz the oracle's compress() of them."""
import io
import tarfile

import pytest

import emu
import oracle
import parity_cases as pc
import synth
import tar_writer_model as twm
from zippy_amd.common import TAR_PLAIN, ZippyError, dfGzip, dfZlib


@pytest.fixture(scope="module")
def eng():
    return emu.engine()


def _blob(n, seed=1):
    return bytes((i * 131 + seed * 7 + (i >> 7)) & 0xFF for i in range(n))


SIZES = [0, 1, 15, 16, 511, 512, 513, 130000]


def _sized_entries():
    return [("f%d.bin" % n, (_blob(n, n), "0", 1600000000 + n)) for n in SIZES]


def test_emu_tar_entry_sizes(eng):
    entries = _sized_entries()
    assert eng.create_tar(entries, TAR_PLAIN) == twm.image(entries)


def test_emu_tar_directories_and_paths(eng):
    entries = [("dir", (b"", "5", 5)), ("dir2", (b"contents of a directory", "5", 6)),
               ("/bin", b"x"), ("a/b/", b"yy"), ("a//b", b"zzz"), ("/", b""),
               ("h" * 154 + "/t", b"head 154"), ("p/" + "t" * 99, b"tail 99"),
               ("q" * 150 + "/" + "r" * 99, _blob(700))]
    img = eng.create_tar(entries, TAR_PLAIN)
    assert img == twm.image(entries)
    with tarfile.open(fileobj=io.BytesIO(img), mode="r:") as tf:
        assert [m.type for m in tf.getmembers()][:2] == [tarfile.DIRTYPE, tarfile.DIRTYPE]


@pytest.mark.parametrize("entries,status", [
    ([], twm.ZH_ERR_TAR_EMPTY),
    ([("h" * 155 + "/t", b"")], twm.ZH_ERR_TAR_PATH),
    ([("t" * 100, b"")], twm.ZH_ERR_TAR_NAME),
    ([("h" * 155 + "/" + "t" * 100, b"")], twm.ZH_ERR_TAR_PATH),
    ([("a", (b"", "2", 0))], twm.ZH_ERR_ARGUMENT),
    ([("a", (b"", "0", -1))], twm.ZH_ERR_ARGUMENT),
    ([("a", (b"", "0", 8 ** 11))], twm.ZH_ERR_ARGUMENT),
    ([("a", b"1"), ("b", b"2"), ("a", b"3")], twm.ZH_ERR_ARGUMENT),
    ([("ok", b"1"), ("t" * 100, b""), ("h" * 155 + "/x", b"")], twm.ZH_ERR_TAR_NAME),
    ([("ok", b"1"), ("a", (b"", "x", 0)), ("t" * 100, b"")], twm.ZH_ERR_ARGUMENT),
])
def test_emu_tar_errors(eng, entries, status):
    assert twm.status(entries) == status
    for fmt in (TAR_PLAIN, dfGzip):
        outs, sts = eng.create_tars([entries], fmt, 1)
        assert outs == [None] and sts == [status]
    with pytest.raises(ZippyError) as ei:
        eng.create_tar(entries, TAR_PLAIN)
    assert ei.value.status == status
    assert eng.lib.zh_strerror(status).decode() == {
        37: "Tarball has no contents", 38: "File path too long, must be < 155 characters",
        39: "File name too long, must be < 100 characters", 22: "Invalid argument"}[status]


def test_emu_tar_call_level_errors(eng):
    with pytest.raises(ZippyError) as ei:
        eng.create_tars([[("a", b"x")]], dfZlib)
    assert ei.value.status == 2  # ZH_ERR_INVALID_FORMAT
    with pytest.raises(ZippyError) as ei:
        eng.create_tars([[("a", b"x")]], dfGzip, 10)
    assert ei.value.status == 1  # ZH_ERR_INVALID_LEVEL
    outs, sts = eng.create_tars([[("a", b"x")]], TAR_PLAIN, 10)  # the level means nothing to a plain image
    assert sts == [0] and outs[0] == twm.image([("a", b"x")])
    assert eng.create_tars([], TAR_PLAIN) == ([], [])


def _raw_tar_call(eng, entries, first, data_format, level):
    """zh_tar_create_batch through ctypes with a hand-made table, poisoned outputs -> (rc, dsts, dst_lens, statuses)"""
    import ctypes as c
    from zippy_amd._binding import TarNewEntry
    n = len(first) - 1
    arr = None if entries is None else (TarNewEntry * len(entries))(*entries)
    dsts = (c.c_void_p * n)(*[0xDEAD000 + 16 * t for t in range(n)])
    dlens, sts = (c.c_size_t * n)(*[12345] * n), (c.c_int32 * n)(*[77] * n)
    rc = eng.lib.zh_tar_create_batch(eng._h, arr, (c.c_size_t * len(first))(*first), n, data_format, level, dsts,
                                     dlens, sts)
    return rc, list(dsts), list(dlens), list(sts)


def _tar_entry(path, contents, path_len=None, length=None):
    """a TarNewEntry with the pointers as given (None: NULL) and the lengths of the data unless given"""
    import ctypes as c
    from zippy_amd._binding import TarNewEntry
    return TarNewEntry(path, len(path or b"") if path_len is None else path_len,
                       c.cast(c.c_char_p(contents), c.c_void_p) if contents else None,
                       len(contents or b"") if length is None else length, b"0", 0)


_GOOD = [(b"a", b"xy"), (b"b", b"z")]


@pytest.mark.parametrize("table,first,fmt,level,rc", [
    (_GOOD, [0, 2, 1], TAR_PLAIN, 1, twm.ZH_ERR_ARGUMENT),  # decreasing first[]
    (_GOOD, [0, 2, 1], dfGzip, 1, twm.ZH_ERR_ARGUMENT),
    (None, [0, 0, 1], dfGzip, 1, twm.ZH_ERR_ARGUMENT),  # entries == NULL with a non-zero count
    ([(b"a", b"xy"), (None, b"z", 1)], [0, 1, 2], TAR_PLAIN, 1, twm.ZH_ERR_ARGUMENT),  # path NULL, path_len 1
    ([(b"a", b"xy"), (b"b", None, None, 5)], [0, 1, 2], dfGzip, 1, twm.ZH_ERR_ARGUMENT),  # contents NULL, len 5
    (_GOOD, [0, 2, 1], dfZlib, 1, 2),  # the format is checked before the table (ZH_ERR_INVALID_FORMAT)
    (_GOOD, [0, 2, 1], dfGzip, 10, 1),  # ... and a .tar.gz's level (ZH_ERR_INVALID_LEVEL)
    (_GOOD, [0, 2, 1], TAR_PLAIN, 10, twm.ZH_ERR_ARGUMENT),  # (a plain image has no level)
    (None, [0, 1], dfZlib, 10, 2),
])
def test_emu_tar_c_level_refusals(eng, table, first, fmt, level, rc):
    entries = None if table is None else [_tar_entry(*e) for e in table]
    n = len(first) - 1
    assert _raw_tar_call(eng, entries, first, fmt, level) == (rc, [None] * n, [0] * n, [0] * n)


def _batch():
    good = [
        [("one.txt", b"hello")],
        _sized_entries()[:7],
        [("d", (b"", "5", 1)), ("d/x", _blob(1000, 3))],
        [("big/" + "b" * 90, _blob(140000, 9))],
    ]
    bad = [[], [("t" * 100, b"")], [("a", b""), ("a", b"")]]
    return [good[0], bad[0], good[1], bad[1], good[2], bad[2], good[3]]


def test_emu_tar_batch_mixes_good_and_bad(eng):
    tars = _batch()
    want_st = [twm.status(t) for t in tars]
    assert sorted(set(want_st)) == [0, twm.ZH_ERR_ARGUMENT, twm.ZH_ERR_TAR_EMPTY, twm.ZH_ERR_TAR_NAME]
    outs, sts = eng.create_tars(tars, TAR_PLAIN)
    assert sts == want_st
    for t, out, st in zip(tars, outs, sts):
        if st == 0:
            assert out == twm.image(t) == eng.create_tar(t, TAR_PLAIN)
        else:
            assert out is None
    gz, sts = eng.create_tars(tars, dfGzip, 1)
    assert sts == want_st
    for t, out, st in zip(tars, gz, sts):
        if st == 0:
            assert out == eng.create_tar(t, dfGzip, 1) == oracle.compress(twm.image(t), 1, oracle.dfGzip, fname_len=0)


def test_emu_tar_gzip_first_cap_retry(eng, monkeypatch):
    """ZH_COMPRESS_FIRST_CAP=64: the images of a mixed batch outgrow their first slots and are compressed again into
    zh_compress_bound slots -- the same bytes as without it, the oracle's compress() of the model's images"""
    tars = _batch()
    want = eng.create_tars(tars, dfGzip, 1)
    monkeypatch.setenv("ZH_COMPRESS_FIRST_CAP", "64")
    assert eng.create_tars(tars, dfGzip, 1) == want
    assert want[1] == [twm.status(t) for t in tars]
    for t, out, st in zip(tars, want[0], want[1]):
        assert out == (oracle.compress(twm.image(t), 1, oracle.dfGzip, fname_len=0) if st == 0 else None)


@pytest.mark.parametrize("level", [-2, 0, 1, -1, 9])
def test_emu_tar_gzip_levels(eng, level):
    entries = _sized_entries()[:7] + [("text/alice.txt", (synth.corpus_file("alice29.txt")[:60000], "0", 99))]
    img = twm.image(entries)
    assert eng.create_tar(entries, dfGzip, level) == oracle.compress(img, level, oracle.dfGzip, fname_len=0)


def test_emu_tar_round_trip(eng):
    entries = [("r/" + str(i), (_blob(37 * i, i), "0", i)) for i in range(40)] + [("r", (b"", "5", 0))]
    gz = eng.create_tar(entries, dfGzip)
    assert pc.check_tarball(eng, gz) == len(entries)
    reader = eng.open_tar(gz)
    assert [e["path"] for e in reader.entries] == [p.encode() for p, _ in entries]
    assert [reader.contents(i) for i in range(len(entries))] == [v[0] for _, v in entries]
    reader.close()
    with tarfile.open(fileobj=io.BytesIO(gz), mode="r:gz") as tf:
        assert [(m.name, m.size, m.mtime) for m in tf.getmembers()] == [(p, len(v[0]), v[2]) for p, v in entries]
