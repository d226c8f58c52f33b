"""CPU-only: zh_tar_read_batch (zippy_amd/csrc/zh_tar_read_batch.hip) under the fiber emulator of tests/hipemu.  Every
status, the key order, every field and every content byte must equal what tests/tar_v1_reader_model.py
(tarballs_v1.nim's openStreamImpl restated) says.
Subsets, where the emulator is slow: the chains run alone and between neighbours up to 600 blocks (the longer ones run
in the one big call here, and every way in the GPU file); the reference's fixture (22 MiB uncompressed, some 44 000
nodes: 40 s a call here) runs once, alone -- between two hand-made images it runs in the GPU file.  Everything else
runs in full."""
import ctypes as c
import random

import pytest

import emu
import tar_read_cases as rc


@pytest.fixture(scope="module")
def eng():
    return emu.engine()


def test_emu_tar_read_chains(eng):
    cases = rc.chains()
    rc.run_cases(eng, [x for x in cases if len(x[1]) <= 600 * 512])
    rc.check_batch(eng, [x[1] for x in cases], [x[2] for x in cases], want=[x[3] for x in cases])


def test_emu_tar_read_chains_share_the_rounds(eng):
    """the round count comes from the call: pairs that straddle a power of two, both orders"""
    for a, b in rc.CHAIN_PAIRS:
        rc.check_batch(eng, [rc.chain(a), rc.chain(b, 1)], want=[0, 0])


FAMILIES = [f for f in rc.families() if f[0] != "chains"]


@pytest.mark.parametrize("name,cases", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_emu_tar_read_family(eng, name, cases):
    """every case alone, between two neighbours, and the family in one call"""
    rc.run_cases(eng, cases)


def test_emu_tar_read_all_cases_in_one_call(eng):
    cases = rc.all_cases()
    rc.check_batch(eng, [x[1] for x in cases], [x[2] for x in cases], want=[x[3] for x in cases])


def test_emu_tar_read_formats_none(eng):
    good = rc.good_images()
    assert rc.check_batch(eng, good + [b"\x1f\0"], None, want=[0, 0, rc.TAR_FORMAT]) == [0, 0, rc.TAR_FORMAT]
    rc.with_error(rc.ARGUMENT, lambda: eng.read_tars(good, [rc.DETECT, 3]))
    rc.with_error(rc.ARGUMENT, lambda: eng.read_tars(good, [-1, rc.GZIP]))
    for bad in ([rc.DETECT], [rc.DETECT] * 3):  # one format an image
        with pytest.raises(ValueError):
            eng.read_tars(good, bad)


def test_emu_tar_read_statuses_have_the_reference_messages(eng):
    assert [eng.lib.zh_strerror(s).decode() for s in (46, 47, 48, 49)] == [
        "Unsupported tarball format", "Unexpected error while opening tarball",
        "Unexpected error while opening tarball (mode)", "Attempted to read past end of file, corrupted tarball?"]


def test_emu_tar_read_round_trips(eng):
    for fmt, data_format in ((rc.PLAIN, -1), (rc.GZIP, 2), (rc.DETECT, 2)):
        outs, sts = eng.create_tars(rc.ROUND_TRIP, data_format, 1)
        assert sts == [0, 0]
        assert rc.check_batch(eng, outs, [fmt, fmt], want=[0, 0]) == [0, 0]
        for image, entries in zip(outs, rc.ROUND_TRIP):
            assert rc.table_rows(rc.tm.expected(image, fmt)[2]) == rc.written(entries)


def test_emu_tar_read_fixture(eng):
    """the reference's libressl-3.4.2.tar.gz (v7 headers), alone"""
    fx = rc.fixture()
    assert rc.check_batch(eng, [fx], want=[0]) == [0]
    assert len(rc.tm.expected(fx)[2]) == 1743


def test_emu_tar_read_mixed(eng):
    images = rc.random_images(20261018, 256)
    rc.check_batch(eng, [x[0] for x in images], [x[1] for x in images])
    for image, fmt in images:  # each alone
        rc.check_batch(eng, [image], [fmt])


def test_emu_tar_read_plumbing(eng):
    assert eng.read_tars([]) == ([], [])
    good = rc.good_images()
    rc.check_batch(eng, [good[1]] * 4, want=[0] * 4)  # the same image four times
    order = list(range(6))
    random.Random(5).shuffle(order)
    rc.check_batch(eng, good * 3, close_order=order)


def _raw(eng, images, lens, n, readers=True, statuses=True, formats=None):
    rd, st = (c.c_void_p * max(n, 1))(*[0xDEAD0] * max(n, 1)), (c.c_int32 * max(n, 1))(*[77] * max(n, 1))
    rc_ = eng.lib.zh_tar_read_batch(eng._h, images, lens, formats, n, rd if readers else None, st if statuses else None)
    return rc_, list(rd)[:n], list(st)[:n]


def test_emu_tar_read_call_level_errors(eng):
    img = rc.good_images()[0]
    ptr = (c.c_void_p * 2)(c.cast(c.c_char_p(img), c.c_void_p), None)
    lens = (c.c_size_t * 2)(len(img), 0)
    assert _raw(eng, ptr, (c.c_size_t * 2)(len(img), 5), 2) == (22, [None, None], [0, 0])  # NULL with a length
    rc_, rd, st = _raw(eng, ptr, lens, 2)  # NULL without one: that image's own status
    assert (rc_, st) == (0, [0, rc.TAR_FORMAT]) and rd[0] and not rd[1]
    eng.lib.zh_tar_close(rd[0])
    rc_, rd, st = _raw(eng, ptr, lens, 2, formats=(c.c_int32 * 2)(rc.DETECT, rc.PLAIN))  # ... an empty tarball
    assert (rc_, st) == (0, [0, 0]) and rd[0] and rd[1] and eng.lib.zh_tar_num_entries(rd[1]) == 0
    eng.lib.zh_tar_close(rd[0])
    eng.lib.zh_tar_close(rd[1])
    assert _raw(eng, ptr, lens, 2, formats=(c.c_int32 * 2)(rc.DETECT, 3)) == (22, [None, None], [0, 0])
    assert _raw(eng, None, None, 2)[0] == 22
    assert _raw(eng, ptr, lens, 2, readers=False) == (22, [0xDEAD0] * 2, [77] * 2)
    assert _raw(eng, ptr, lens, 2, statuses=False) == (22, [0xDEAD0] * 2, [77] * 2)
    assert _raw(eng, None, None, 0, readers=False, statuses=False)[0] == 0
    assert eng.lib.zh_tar_read_batch(None, ptr, lens, None, 2, (c.c_void_p * 2)(), (c.c_int32 * 2)()) == 22
