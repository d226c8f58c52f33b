"""CPU-only: zh_tar_open_batch (zippy_amd/csrc/zh_tar_open_batch.hip) under the fiber emulator of tests/hipemu.  Every
status, every uncompressed image and every field of every entry must equal what oracle/tar_oracle.py's open_tarball
(tarballs.nim restated) and Engine.open_tar on the image alone say.  Plain .tar images, plus a few small .tar.gz."""
import ctypes as c
import random

import pytest

import emu
import tar_open_cases as tc


@pytest.fixture(scope="module")
def eng():
    return emu.engine()


def _ids(cases):
    return [x[0] for x in cases]


def test_emu_tar_open_doubling_chains(eng):
    """chains of 1, 2, 3 and 2^k - 1, 2^k, 2^k + 1 headers (k = 2..11), each by itself: its own round count"""
    for name, image in tc.doubling_chains():
        sts = tc.check_batch(eng, [image], want=[0], second_referee=False)
        assert sts == [0], name
        assert len(tc.expected(image)[2]) == len(image) // 512


def test_emu_tar_open_chains_share_the_rounds(eng):
    """the round count comes from the largest image of the call: chains that straddle a power of two, both orders"""
    chains = dict(tc.doubling_chains())
    for a, b in [(127, 129), (129, 127), (1, 2049), (2048, 3), (255, 256)]:
        tc.check_batch(eng, [chains["chain%d" % a], chains["chain%d" % b]], want=[0, 0], second_referee=False)
    tc.check_batch(eng, [image for _, image in tc.doubling_chains()][:20], second_referee=False)


@pytest.mark.parametrize("name,image", tc.doubling_shapes() + tc.decoys() + tc.walk_semantics() + tc.statuses_fine(),
                         ids=_ids(tc.doubling_shapes() + tc.decoys() + tc.walk_semantics() + tc.statuses_fine()))
def test_emu_tar_open_walk(eng, name, image):
    """shapes of the walk, decoys inside contents, the reference's handling of magic, prefix, types and long names:
    all of them open, alone and between neighbours"""
    assert tc.check_batch(eng, [image], want=[0]) == [0]
    good = tc.good_images()
    zipped = image if image[:2] == b"\x1f\x8b" else tc.gz(image)
    tc.check_batch(eng, [good[0], image, zipped, good[1]], want=[0, 0, 0, 0], second_referee=False)


def test_emu_tar_open_decoys_report_only_their_own(eng):
    readers, sts = eng.open_tars([image for _, image in tc.decoys()])
    assert sts == [0, 0, 0]
    assert [[e["path"] for e in r.entries] for r in readers] == [
        [b"inner.tar", b"after"], [b"nines", b"eights", b"e0", b"e1"], [b"inner.tar", b"e0"]]


def test_emu_tar_open_formats(eng):
    """Python's tarfile in USTAR, GNU and PAX formats, plain and gzipped, in one call"""
    good = tc.good_images()
    assert tc.check_batch(eng, good + [tc.gz(g) for g in good], want=[0] * 6) == [0] * 6
    # GNU format: every name arrives whole ('L' blocks); USTAR cannot hold them all, PAX keeps them in 'x' blocks
    assert [e["path"].rstrip(b"\0") for e in tc.expected(good[1])[2]] == [
        m[0].encode() + (b"/" if m[1] is None else b"") for m in tc.MEMBERS]


@pytest.mark.parametrize("name,image,status", tc.statuses(), ids=_ids(tc.statuses()))
def test_emu_tar_open_status(eng, name, image, status):
    """every status, alone in a batch whose neighbours succeed"""
    good = tc.good_images()
    assert tc.check_batch(eng, [good[0], image, good[1]], want=[0, status, 0]) == [0, status, 0]
    assert eng.lib.zh_strerror(status).decode() == {
        13: "Invalid buffer, unable to uncompress", 23: "Unexpected EOF, invalid archive?",
        34: "Unsupported header type", 35: "Path not allowed (absolute or containing ../)",
        36: "Invalid octal number in tar header", 8: "Checksum verification failed", 9: "Size verification failed"}[status]


@pytest.mark.parametrize("name,image,status", tc.precedence(), ids=_ids(tc.precedence()))
def test_emu_tar_open_precedence(eng, name, image, status):
    """the earlier header's fault wins; within a header: numbers, EOF, path, type; a fault behind the first is invisible"""
    good = tc.good_images()
    assert tc.check_batch(eng, [image, good[2], image], want=[status, 0, status]) == [status, 0, status]


def test_emu_tar_open_plumbing(eng):
    assert eng.open_tars([]) == ([], [])
    good = tc.good_images()
    tc.check_batch(eng, [good[1], good[1], tc.gz(good[1]), tc.gz(good[1])], want=[0] * 4)  # the same image twice
    order = list(range(6))
    random.Random(5).shuffle(order)
    tc.check_batch(eng, good + [tc.gz(g) for g in good], close_order=order, second_referee=False)
    tc.check_batch(eng, [b"", b"x", b"\x1f\x8b"], want=[13, 13, 13])  # nothing reaches the device


def test_emu_tar_open_256_mixed(eng):
    images = tc.random_images(20261017, 256, 0.06)
    sts = tc.check_batch(eng, images)
    assert sts.count(0) > 128 and len(set(sts)) >= 4, sorted(set(sts))


def _raw(eng, images, lens, n, readers=True, statuses=True):
    rd, st = (c.c_void_p * max(n, 1))(*[0xDEAD0] * max(n, 1)), (c.c_int32 * max(n, 1))(*[77] * max(n, 1))
    rc = eng.lib.zh_tar_open_batch(eng._h, images, lens, n, rd if readers else None, st if statuses else None)
    return rc, list(rd)[:n], list(st)[:n]


def test_emu_tar_open_call_level_errors(eng):
    img = tc.good_images()[0]
    ptr = (c.c_void_p * 2)(c.cast(c.c_char_p(img), c.c_void_p), None)
    assert _raw(eng, ptr, (c.c_size_t * 2)(len(img), 5), 2) == (22, [None, None], [0, 0])  # NULL with a length
    rc, rd, st = _raw(eng, ptr, (c.c_size_t * 2)(len(img), 0), 2)  # NULL without one: that image's own status
    assert (rc, st) == (0, [0, 13]) and rd[0] and not rd[1]
    eng.lib.zh_tar_close(rd[0])
    assert _raw(eng, None, None, 2)[0] == 22
    assert _raw(eng, ptr, (c.c_size_t * 2)(len(img), 0), 2, readers=False)[0] == 22
    assert _raw(eng, ptr, (c.c_size_t * 2)(len(img), 0), 2, statuses=False)[0] == 22
    assert _raw(eng, None, None, 0, readers=False, statuses=False)[0] == 0
    assert eng.lib.zh_tar_open_batch(None, ptr, (c.c_size_t * 2)(len(img), 0), 2, (c.c_void_p * 2)(),
                                     (c.c_int32 * 2)()) == 22
