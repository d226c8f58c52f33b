"""CPU-only: zh_zip_open_all_batch (zippy_amd/csrc/zh_zip_open_batch.hip) under the fiber emulator of tests/hipemu.
Every archive status, every field of every entry, every entry status and every extracted byte must equal what
oracle/zip_oracle.py (ziparchives.nim restated) and Engine.open_zip / extract_batch on the image alone say.
Subsets, where the emulator is slow: the doubling chains run alone up to 2^8 + 1 records and all together only in
the GPU file (the 2^11 chains run in one pair here); the alignment archives and the Bagnon fixture run without the
second referee's per-image calls where noted.  The 256 mixed archives run in full, in one call and each alone."""
import ctypes as c
import random

import pytest

import emu
import zip_open_cases as zc
from zippy_amd.common import ZippyError


@pytest.fixture(scope="module")
def eng():
    return emu.engine()


def _ids(cases):
    return [x[0] for x in cases]


def test_emu_zip_open_doubling_chains(eng):
    """archives of 1, 2, 3 and 2^k - 1, 2^k, 2^k + 1 records, each by itself: its own round count; 0 records"""
    for name, image in zc.doubling_chains():
        if len(zc.expected(image)[1]) > 257:
            continue
        assert zc.check_batch(eng, [image], want=[0], second_referee=False) == [0], name
    assert zc.check_batch(eng, [zc.build([])], want=[0]) == [0]


def test_emu_zip_open_chains_share_the_rounds(eng):
    """the round count comes from the largest archive of the call: pairs that straddle a power of two, both orders"""
    chains = dict(zc.doubling_chains())
    for a, b in [(127, 129), (129, 127), (1, 2049), (255, 256)]:
        zc.check_batch(eng, [chains["chain%d" % a], chains["chain%d" % b]], want=[0, 0], second_referee=False)


@pytest.mark.parametrize("name,image,status", zc.geometry() + zc.zip64_cases() + zc.names(),
                         ids=_ids(zc.geometry() + zc.zip64_cases() + zc.names()))
def test_emu_zip_open_records(eng, name, image, status):
    """record geometry, zip64 fields, names: alone between two neighbours that open"""
    good = zc.good_images()
    sts = zc.check_batch(eng, [good[0], image, good[2]], want=[0, status, 0])
    assert sts[0] == sts[2] == 0


@pytest.mark.parametrize("name,image", zc.decoys() + zc.prefix_suffix(), ids=_ids(zc.decoys() + zc.prefix_suffix()))
def test_emu_zip_open_decoys_and_prefixes(eng, name, image):
    good = zc.good_images()
    zc.check_batch(eng, [good[1], image, good[0]], want=[0, None, 0])


def test_emu_zip_open_decoys_report_only_their_own(eng):
    cases = dict(zc.decoys())
    readers, sts = eng.open_zips([cases["in_stored_data"], cases["in_stored_data_prefixed"]])
    assert sts == [0, 0]
    assert [[e["path"] for e in r.entries] for r in readers] == [["a", "data.bin", "c"]] * 2
    assert all(b"decoy.txt" in r.contents(1) for r in readers)


@pytest.mark.parametrize("name,image,status", zc.open_statuses() + zc.precedence(),
                         ids=_ids(zc.open_statuses() + zc.precedence()))
def test_emu_zip_open_status(eng, name, image, status):
    """every open status and the serial loop's precedence, alone between two neighbours that open"""
    good = zc.good_images()
    sts = zc.check_batch(eng, [good[0], image, good[1]], want=[0, status, 0])
    assert sts[0] == sts[2] == 0 and (status is None or sts[1] == status)


def test_emu_zip_open_statuses_in_one_call(eng):
    cases = zc.open_statuses() + zc.precedence()
    zc.check_batch(eng, [x[1] for x in cases], want=[x[2] for x in cases], second_referee=False)


@pytest.mark.parametrize("name,image,status", zc.entry_statuses(), ids=_ids(zc.entry_statuses()))
def test_emu_zip_open_entry_status(eng, name, image, status):
    """one damaged file entry: the archive's status is the first failing file entry's, everything else is intact"""
    good = zc.good_images()
    sts = zc.check_batch(eng, [good[2], image, good[1]], want=[0, status, 0])
    assert sts[0] == sts[2] == 0


@pytest.mark.parametrize("name,image", zc.alignment(), ids=_ids(zc.alignment()))
def test_emu_zip_open_alignment(eng, name, image):
    assert zc.check_batch(eng, [image], want=[0], second_referee=False) == [0]
    if name == "method0":  # the multi-chunk copy runs at every shift between source and slot
        assert zc.copy_shifts(eng, image) == set(range(16))


def test_emu_zip_open_plumbing(eng):
    assert eng.open_zips([]) == ([], [])
    good = zc.good_images()
    zc.check_batch(eng, [good[1]] * 4, want=[0] * 4)  # the same image four times
    order = list(range(6))
    random.Random(5).shuffle(order)
    zc.check_batch(eng, good + good, close_order=order, second_referee=False)
    readers, sts = eng.open_zips([good[0]])
    r = readers[0]
    try:  # an ordinary reader: zh_zip_find, zh_zip_extract_batch
        i = r.find("dir/b.bin")
        assert r.extract_batch([i]) == ([zc.blob(3000)], [0]) and r.contents(i) == zc.blob(3000)
        assert r.extract_file("dir/a.txt") == b"alpha" * 40
    finally:
        r.close()
    plain = eng.open_zip(good[0])
    try:
        assert plain.data == b""
        with pytest.raises(ZippyError) as err:
            plain.entry_status(0)
        assert err.value.status == zc.ARGUMENT
    finally:
        plain.close()


def test_emu_zip_open_mixed_generator_is_mixed():
    """the 256 mixed archives by the oracle alone: more than half open, at least 5 statuses"""
    sts = [zc.expected(image)[0] for image in zc.random_images(20261018, 256)]
    opened = sum(1 for image in zc.random_images(20261018, 256) if zc.expected(image)[1] is not None)
    assert opened > 128 and len(set(sts)) >= 5, (opened, sorted(set(sts)))


def test_emu_zip_open_mixed(eng):
    images = zc.random_images(20261018, 256)
    zc.check_batch(eng, images, second_referee=False)
    for t, image in enumerate(images):  # each alone, with the second referee
        zc.check_batch(eng, [image])


def test_emu_zip_open_bagnon(eng):
    image = zc.bagnon()
    good = zc.good_images()
    assert zc.check_batch(eng, [image], want=[0]) == [0]
    assert zc.check_batch(eng, [good[0], image, good[1]], want=[0, 0, 0], second_referee=False) == [0, 0, 0]


def _raw(eng, images, lens, n, readers=True, statuses=True):
    rd, st = (c.c_void_p * max(n, 1))(*[0xDEAD0] * max(n, 1)), (c.c_int32 * max(n, 1))(*[77] * max(n, 1))
    rc = eng.lib.zh_zip_open_all_batch(eng._h, images, lens, n, rd if readers else None, st if statuses else None)
    return rc, list(rd)[:n], list(st)[:n]


def test_emu_zip_open_call_level_errors(eng):
    img = zc.good_images()[0]
    ptr = (c.c_void_p * 2)(c.cast(c.c_char_p(img), c.c_void_p), None)
    assert _raw(eng, ptr, (c.c_size_t * 2)(len(img), 5), 2) == (22, [None, None], [0, 0])  # NULL with a length
    rc, rd, st = _raw(eng, ptr, (c.c_size_t * 2)(len(img), 0), 2)  # NULL without one: that image's own status
    assert (rc, st) == (0, [0, zc.ARCHIVE_EOF]) and rd[0] and not rd[1]
    n, data, ln, est = c.c_size_t(), c.c_void_p(), c.c_size_t(), c.c_int32()
    assert eng.lib.zh_zip_entry_data(rd[0], 10 ** 6, c.byref(data), c.byref(ln), c.byref(est)) == 22
    assert eng.lib.zh_zip_entry_data(rd[0], 0, None, c.byref(ln), c.byref(est)) == 22
    assert eng.lib.zh_zip_entry_data(None, 0, c.byref(data), c.byref(ln), c.byref(est)) == 22
    assert eng.lib.zh_zip_data(None, c.byref(n)) is None and n.value == 0
    eng.lib.zh_zip_close(rd[0])
    assert _raw(eng, None, None, 2)[0] == 22
    assert _raw(eng, ptr, (c.c_size_t * 2)(len(img), 0), 2, readers=False)[0] == 22
    assert _raw(eng, ptr, (c.c_size_t * 2)(len(img), 0), 2, statuses=False)[0] == 22
    assert _raw(eng, None, None, 0, readers=False, statuses=False)[0] == 0
    assert eng.lib.zh_zip_open_all_batch(None, ptr, (c.c_size_t * 2)(len(img), 0), 2, (c.c_void_p * 2)(),
                                         (c.c_int32 * 2)()) == 22
