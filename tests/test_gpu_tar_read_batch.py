"""zh_tar_read_batch on a real MI355X (-m gpu): the cases of tests/tar_read_cases.py on the device, in full.  Every
status, the key order, every field and every content byte against tests/tar_v1_reader_model.py (tarballs_v1.nim's
openStreamImpl restated); every decoder verdict against Engine.uncompress_batch on the same bytes."""
import ctypes as c
import random

import pytest

import tar_read_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch  # torch's bundled HIP runtime has to initialise before libzippy_hip.so's
    torch.cuda.init()
    from zippy_amd import api
    e = api.engine()
    e.set_gzip_fname_len(0)
    return e


def test_gpu_tar_read_chains(eng):
    """1, 2, 3 and 2^k - 1, 2^k, 2^k + 1 named headers (k = 2..11), plain and with runs of nameless blocks between
    them; images of zero blocks only; the empty image: each alone (its own round count), between neighbours, all in
    one call; pairs that straddle a power of two in one call, in both orders"""
    rc.run_cases(eng, rc.chains())
    for a, b in rc.CHAIN_PAIRS:
        rc.check_batch(eng, [rc.chain(a), rc.chain(b, 1)], want=[0, 0])
        rc.check_batch(eng, [rc.chain(a, 2), rc.chain(b)], want=[0, 0])


def test_gpu_tar_read_ends(eng):
    rc.run_cases(eng, rc.ends())


def test_gpu_tar_read_decoys(eng):
    rc.run_cases(eng, rc.decoys())
    cases = {x[0]: x[1] for x in rc.decoys()}
    readers, sts = eng.read_tars([cases["nameless_size_is_not_jumped"], cases["lookalikes_in_contents"]])
    try:
        assert sts == [0, 0]
        assert [[e["path"] for e in r.entries] for r in readers] == [[b"in1", b"in2", b"in3"], [b"inner.tar", b"after"]]
    finally:
        for r in readers:
            r.close()


def test_gpu_tar_read_number_parsing(eng):
    rc.run_cases(eng, rc.number_parsing())
    cases = {x[0]: x[1] for x in rc.number_parsing()}
    readers, sts = eng.read_tars([cases["mode_seventh_byte_digit"], cases["mode_v7"], cases["size_0o_small"]])
    try:
        assert sts == [0, 0, 0]
        assert [readers[0].entries[0]["mode"], readers[1].entries[0]["mode"]] == [0o64, 0o100664]
        assert readers[2].contents(1) == b"12345678"
    finally:
        for r in readers:
            r.close()


def test_gpu_tar_read_precedence(eng):
    rc.run_cases(eng, rc.precedence())


def test_gpu_tar_read_magic_and_join(eng):
    rc.run_cases(eng, rc.magic_and_join())


def test_gpu_tar_read_keys(eng):
    rc.run_cases(eng, rc.keys())
    cases = {x[0]: x[1] for x in rc.keys()}
    readers, sts = eng.read_tars([cases["repeated_key"], cases["file_then_directory"]])
    try:
        assert sts == [0, 0]
        assert [(e["path"], e["mtime"], e["mode"]) for e in readers[0].entries] == [
            (b"k", 2, 0o600), (b"m", 0o14000000000, 0o64), (b"z", 0o14000000000, 0o64)]
        assert readers[0].contents(0) == b"22"
        assert [(e["path"], e["typeflag"], e["size"], e["offset"], e["mtime"], e["mode"]) for e in readers[1].entries] == [
            (b"k", b"5", 0, 0, 0, 0), (b"o", b"0", 1, 3 * 512, 0o14000000000, 0o64)]
    finally:
        for r in readers:
            r.close()


def test_gpu_tar_read_type_flags(eng):
    rc.run_cases(eng, rc.type_flags())


def test_gpu_tar_read_formats(eng):
    rc.run_cases(eng, rc.formats())
    good = rc.good_images()
    assert rc.check_batch(eng, good + [b"\x1f\0"], None, want=[0, 0, rc.TAR_FORMAT]) == [0, 0, rc.TAR_FORMAT]
    rc.with_error(rc.ARGUMENT, lambda: eng.read_tars(good, [rc.DETECT, 3]))
    rc.with_error(rc.ARGUMENT, lambda: eng.read_tars(good, [-1, rc.GZIP]))
    assert [eng.lib.zh_strerror(s).decode() for s in (46, 47, 48, 49)] == [
        "Unsupported tarball format", "Unexpected error while opening tarball",
        "Unexpected error while opening tarball (mode)", "Attempted to read past end of file, corrupted tarball?"]


def test_gpu_tar_read_gzips(eng):
    rc.run_cases(eng, rc.gzips())


def test_gpu_tar_read_round_trips(eng):
    """create_tars -> read_tars for .tar and .tar.gz, two tarballs a call"""
    for fmt, data_format in ((rc.PLAIN, -1), (rc.GZIP, 2), (rc.DETECT, 2)):
        for level in (1, -1):
            outs, sts = eng.create_tars(rc.ROUND_TRIP, data_format, level)
            assert sts == [0, 0]
            assert rc.check_batch(eng, outs, [fmt, fmt], want=[0, 0]) == [0, 0]
            for image, entries in zip(outs, rc.ROUND_TRIP):
                assert rc.table_rows(rc.tm.expected(image, fmt)[2]) == rc.written(entries)


def test_gpu_tar_read_fixture(eng):
    """the reference's libressl-3.4.2.tar.gz (v7 headers; 22 MiB uncompressed): alone, and between two hand-made images"""
    fx, good = rc.fixture(), rc.good_images()
    assert rc.check_batch(eng, [fx], want=[0]) == [0]
    assert len(rc.tm.expected(fx)[2]) == 1743
    assert rc.check_batch(eng, [good[0], fx, good[1]], [rc.DETECT, rc.GZIP, rc.GZIP], want=[0, 0, 0]) == [0, 0, 0]


def test_gpu_tar_read_all_cases_in_one_call(eng):
    cases = rc.all_cases()
    rc.check_batch(eng, [x[1] for x in cases], [x[2] for x in cases], want=[x[3] for x in cases])


def test_gpu_tar_read_mixed(eng):
    images = rc.random_images(20261018, 256)
    rc.check_batch(eng, [x[0] for x in images], [x[1] for x in images])
    for image, fmt in images:  # each alone
        rc.check_batch(eng, [image], [fmt])


def test_gpu_tar_read_plumbing(eng):
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


def test_gpu_tar_read_call_level_errors(eng):
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
