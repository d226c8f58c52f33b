"""zh_zip_open_all_batch on a real MI355X (-m gpu): the cases of tests/test_emu_zip_open_batch.py on the device, in
full.  Every archive status, every field of every entry, every entry status and every extracted byte against
oracle/zip_oracle.py and against Engine.open_zip / extract_batch on the image alone."""
import ctypes as c
import random

import pytest

import zip_open_cases as zc
from zippy_amd.common import ZippyError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch  # torch's bundled HIP runtime has to initialise before libzippy_hip.so's
    torch.cuda.init()
    from zippy_amd import api
    e = api.engine()
    e.set_gzip_fname_len(0)
    return e


def test_gpu_zip_open_doubling_chains(eng):
    """archives of 0, 1, 2, 3 and 2^k - 1, 2^k, 2^k + 1 records (k = 2..11): each by itself (its own round count),
    pairs that straddle a power of two in both orders (the round count comes from the larger), all in one call"""
    chains = zc.doubling_chains()
    for name, image in chains:
        assert zc.check_batch(eng, [image], want=[0], second_referee=False) == [0], name
    assert zc.check_batch(eng, [zc.build([])], want=[0]) == [0]
    by_name = dict(chains)
    for a, b in [(127, 129), (129, 127), (1, 2049), (2048, 3), (255, 256)]:
        zc.check_batch(eng, [by_name["chain%d" % a], by_name["chain%d" % b]], want=[0, 0], second_referee=False)
    zc.check_batch(eng, [image for _, image in chains] + [zc.build([])], second_referee=False)


def test_gpu_zip_open_records(eng):
    """record geometry, zip64 fields, names: each between two neighbours that open, then all in one call"""
    good = zc.good_images()
    cases = zc.geometry() + zc.zip64_cases() + zc.names()
    for name, image, status in cases:
        sts = zc.check_batch(eng, [good[0], image, good[2]], want=[0, status, 0])
        assert sts[0] == sts[2] == 0, name
    zc.check_batch(eng, [x[1] for x in cases], want=[x[2] for x in cases], second_referee=False)


def test_gpu_zip_open_decoys_and_prefixes(eng):
    good = zc.good_images()
    for name, image in zc.decoys() + zc.prefix_suffix():
        zc.check_batch(eng, [good[1], image, good[0]], want=[0, None, 0])
    cases = dict(zc.decoys())
    readers, sts = eng.open_zips([cases["in_stored_data"], cases["in_stored_data_prefixed"]])
    assert sts == [0, 0]
    assert [[e["path"] for e in r.entries] for r in readers] == [["a", "data.bin", "c"]] * 2
    assert all(b"decoy.txt" in r.contents(1) for r in readers)
    for r in readers:
        r.close()


def test_gpu_zip_open_statuses(eng):
    """every open status and the serial loop's precedence: alone between two neighbours that open, then all in one call"""
    good = zc.good_images()
    cases = zc.open_statuses() + zc.precedence()
    for name, image, status in cases:
        sts = zc.check_batch(eng, [good[0], image, good[1]], want=[0, status, 0])
        assert sts[0] == sts[2] == 0 and (status is None or sts[1] == status), name
    zc.check_batch(eng, [x[1] for x in cases], want=[x[2] for x in cases], second_referee=False)


def test_gpu_zip_open_entry_statuses(eng):
    """one damaged file entry: the archive's status is the first failing file entry's, everything else is intact"""
    good = zc.good_images()
    cases = zc.entry_statuses()
    for name, image, status in cases:
        sts = zc.check_batch(eng, [good[2], image, good[1]], want=[0, status, 0])
        assert sts[0] == sts[2] == 0, name
    zc.check_batch(eng, [x[1] for x in cases], want=[x[2] for x in cases], second_referee=False)


def test_gpu_zip_open_alignment(eng):
    for name, image in zc.alignment():
        assert zc.check_batch(eng, [image], want=[0]) == [0], name
        if name == "method0":  # the multi-chunk copy runs at every shift between source and slot
            assert zc.copy_shifts(eng, image) == set(range(16))


def test_gpu_zip_open_plumbing(eng):
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


def test_gpu_zip_open_256_mixed(eng):
    images = zc.random_images(20261018, 256)
    sts = zc.check_batch(eng, images, second_referee=False)
    opened = sum(1 for image in images if zc.expected(image)[1] is not None)
    assert opened > 128 and len(set(sts)) >= 5, (opened, sorted(set(sts)))
    for lo in range(0, 256, 64):  # with the second referee
        zc.check_batch(eng, images[lo:lo + 64])


def test_gpu_zip_open_bagnon(eng):
    """the reference's fixture, alone and in the middle of a batch, and through the API"""
    from zippy_amd import api
    image = zc.bagnon()
    good = zc.good_images()
    assert zc.check_batch(eng, [image], want=[0]) == [0]
    assert zc.check_batch(eng, [good[0], image, good[1]], want=[0, 0, 0], second_referee=False) == [0, 0, 0]
    readers = api.openZipArchives([good[0], image])
    try:
        st, entries, results = zc.expected(image)
        assert readers[1].entries == entries
        assert [readers[1].contents(i) for i in range(len(entries))] == [data for _, data in results]
    finally:
        for r in readers:
            r.close()
    with pytest.raises(ZippyError) as err:
        api.openZipArchives([good[0], image[:len(image) // 2], good[1]])
    assert err.value.status == zc.ARCHIVE_EOF


def _raw(eng, images, lens, n, readers=True, statuses=True):
    rd, st = (c.c_void_p * max(n, 1))(*[0xDEAD0] * max(n, 1)), (c.c_int32 * max(n, 1))(*[77] * max(n, 1))
    rc = eng.lib.zh_zip_open_all_batch(eng._h, images, lens, n, rd if readers else None, st if statuses else None)
    return rc, list(rd)[:n], list(st)[:n]


def test_gpu_zip_open_call_level_errors(eng):
    """NULL arguments: the return value alone, nothing launched, nothing handed out"""
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
