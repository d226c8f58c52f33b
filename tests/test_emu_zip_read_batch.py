"""CPU-only: zh_zip_read_batch (zippy_amd/csrc/zh_zip_read_batch.hip) under the fiber emulator of tests/hipemu.
Every status, the key order, every field, every entry_v1 triple and every byte must equal what
tests/zip_v1_reader_model.py (ziparchives_v1.nim's openStreamImpl restated) says.
Subsets, where the emulator is slow: the chains run alone up to 2^8 + 1 local records (the longer ones, and all
chains in one call, run in the GPU file; the 2^11 chains run in one pair here); of the scan geometry's positions
around k x chunk, k = 2 runs only in the GPU file's single call.  Everything else runs in full."""
import ctypes as c
import random

import pytest

import emu
import zip_read_cases as zc
import zip_v1_reader_model as zm


@pytest.fixture(scope="module")
def eng():
    return emu.engine()


def _ids(cases):
    return [x[0] for x in cases]


GEOMETRY = [x for x in zc.scan_geometry() if "_at_2x" not in x[0]]


@pytest.mark.parametrize("name,image,status", GEOMETRY, ids=_ids(GEOMETRY))
def test_emu_zip_read_scan_geometry(eng, name, image, status):
    """alone (the image's positions are the upload's: the scan's own chunk borders) and between two neighbours"""
    assert zc.check_batch(eng, [image], want=[status]) == [status]
    assert zc.alone_between_neighbours(eng, image, status) == status


def test_emu_zip_read_straddling_pair(eng):
    (_, a, sa), (_, b, sb) = zc.straddling_pair()
    assert zc.check_batch(eng, [a, b], want=[sa, sb]) == [sa, sb]
    good = zc.good_images()
    assert zc.check_batch(eng, [a, b, good[0], a, good[1]], want=[sa, sb, 0, sa, 0]) == [sa, sb, 0, sa, 0]


def test_emu_zip_read_chains(eng):
    """0, 1, 2, 3 and 2^k - 1, 2^k, 2^k + 1 local records, each alone: its own round count"""
    for name, image, _ in zc.chains():
        if len(image) <= 46 * 2 * 257 + 22:
            assert zc.check_batch(eng, [image], want=[0]) == [0], name


def test_emu_zip_read_chains_share_the_rounds(eng):
    """the round count comes from the call: pairs that straddle a power of two, both orders"""
    for a, b in [(127, 129), (129, 127), (1, 2049), (255, 256)]:
        zc.check_batch(eng, [zc.chain(a, False), zc.chain(b, True)], want=[0, 0])


@pytest.mark.parametrize("name,image,status", zc.decoys(), ids=_ids(zc.decoys()))
def test_emu_zip_read_decoys(eng, name, image, status):
    zc.alone_between_neighbours(eng, image, status)


@pytest.mark.parametrize("name,image,status", zc.statuses() + zc.tables(), ids=_ids(zc.statuses() + zc.tables()))
def test_emu_zip_read_status(eng, name, image, status):
    """every status, the precedence inside a record and along the walk, the table's rules: alone between neighbours"""
    zc.alone_between_neighbours(eng, image, status)


def test_emu_zip_read_sizes(eng):
    cases = {x[0]: x[1] for x in zc.statuses()}
    readers, sts = eng.read_zips([cases["deflated_csize_0"], cases["usize_ffffffff_tiny_image"]])
    assert sts == [13, zc.SIZE] and readers == [None, None]  # ZH_ERR_INVALID_BUFFER, as the oracle says


def test_emu_zip_read_cases_in_one_call(eng):
    cases = GEOMETRY + zc.straddling_pair() + zc.decoys() + zc.statuses() + zc.tables()
    zc.check_batch(eng, [x[1] for x in cases], want=[x[2] for x in cases])


def test_emu_zip_read_alignment(eng):
    image = zc.alignment()
    readers, sts = eng.read_zips([image])
    try:
        assert sts == [0] and zc.copy_shifts(image, readers[0]) == set(range(16))
    finally:
        readers[0].close()
    assert zc.check_batch(eng, [image], want=[0]) == [0]


def test_emu_zip_read_round_trips(eng):
    entries = [("d/", (b"", True, 0x6000, 0x5521)), ("e", b""), ("h.txt", (b"Hello, World!", False, 7, 9)),
               ("big.bin", zc.blob(40000, 3)), (".hidden", b"stored by its name")]
    for level in (-2, 0, 1, -1, 9):
        outs, sts = eng.write_zips([entries, entries[2:]], level)
        assert sts == [0, 0]
        assert zc.check_batch(eng, outs, want=[0, 0]) == [0, 0]
        table = zm.expected(outs[0])[1]
        assert [(k.decode(), v["contents"]) for k, v in table.items()] == [
            (p, v[0] if isinstance(v, tuple) else v) for p, v in entries]
    outs, sts = eng.create_zips([[("k/x.txt", b"x" * 999), ("k/z", b"")]])
    assert sts == [0] and zc.check_batch(eng, outs, want=[zc.ARCHIVE_EOF]) == [zc.ARCHIVE_EOF]


def test_emu_zip_read_fixtures(eng):
    good = zc.good_images()
    want = [0, zc.DEFLATE64, zc.OPEN, 0]
    assert zc.check_batch(eng, [good[0], zc.fixture("Bagnon-10.2.31.zip"), zc.fixture("cat.jpg"), good[1]], want) == want


def test_emu_zip_read_mixed(eng):
    images = zc.random_images(20261018, 256)
    zc.check_batch(eng, images)
    for image in images:  # each alone
        zc.check_batch(eng, [image])


def test_emu_zip_read_plumbing(eng):
    assert eng.read_zips([]) == ([], [])
    good = zc.good_images()
    zc.check_batch(eng, [good[1]] * 4, want=[0] * 4)  # the same image four times
    order = list(range(6))
    random.Random(5).shuffle(order)
    zc.check_batch(eng, good * 3, close_order=order)
    for plain in (eng.open_zip(good[0]), eng.open_zips([good[0]])[0][0]):  # readers of the other calls
        try:
            zc.with_error(zc.ARGUMENT, lambda: plain.entry_v1(0))
        finally:
            plain.close()
    t, d, i = c.c_uint16(), c.c_uint16(), c.c_int()
    assert eng.lib.zh_zip_entry_v1(None, 0, c.byref(t), c.byref(d), c.byref(i)) == zc.ARGUMENT


def _raw(eng, images, lens, n, readers=True, statuses=True):
    rd, st = (c.c_void_p * max(n, 1))(*[0xDEAD0] * max(n, 1)), (c.c_int32 * max(n, 1))(*[77] * max(n, 1))
    rc = eng.lib.zh_zip_read_batch(eng._h, images, lens, n, rd if readers else None, st if statuses else None)
    return rc, list(rd)[:n], list(st)[:n]


def test_emu_zip_read_call_level_errors(eng):
    img = zc.good_images()[0]
    ptr = (c.c_void_p * 2)(c.cast(c.c_char_p(img), c.c_void_p), None)
    assert _raw(eng, ptr, (c.c_size_t * 2)(len(img), 5), 2) == (22, [None, None], [0, 0])  # NULL with a length
    rc, rd, st = _raw(eng, ptr, (c.c_size_t * 2)(len(img), 0), 2)  # NULL without one: that image's own status
    assert (rc, st) == (0, [0, zc.ARCHIVE_EOF]) and rd[0] and not rd[1]
    eng.lib.zh_zip_close(rd[0])
    assert _raw(eng, None, None, 2)[0] == 22
    assert _raw(eng, ptr, (c.c_size_t * 2)(len(img), 0), 2, readers=False) == (22, [0xDEAD0] * 2, [77] * 2)
    assert _raw(eng, ptr, (c.c_size_t * 2)(len(img), 0), 2, statuses=False) == (22, [0xDEAD0] * 2, [77] * 2)
    assert _raw(eng, None, None, 0, readers=False, statuses=False)[0] == 0
    assert eng.lib.zh_zip_read_batch(None, ptr, (c.c_size_t * 2)(len(img), 0), 2, (c.c_void_p * 2)(),
                                     (c.c_int32 * 2)()) == 22
