"""zh_tar_open_batch on a real MI355X (-m gpu): the cases of tests/test_emu_tar_open_batch.py on the device, plus the
reference's fixture.  Every status, every uncompressed image and every field of every entry against
oracle/tar_oracle.py's open_tarball and against Engine.open_tar on the image alone."""
import random

import pytest

import synth
import tar_open_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch  # torch's bundled HIP runtime has to initialise before libzippy_hip.so's
    torch.cuda.init()
    from zippy_amd import api
    e = api.engine()
    e.set_gzip_fname_len(0)
    return e


def test_gpu_tar_open_doubling_chains(eng):
    """chains of 1, 2, 3 and 2^k - 1, 2^k, 2^k + 1 headers (k = 2..11): each by itself (its own round count), then
    pairs that straddle a power of two (the round count comes from the larger), then all in one call"""
    chains = tc.doubling_chains()
    for name, image in chains:
        assert tc.check_batch(eng, [image], want=[0], second_referee=False) == [0], name
        assert len(tc.expected(image)[2]) == len(image) // 512
    by_name = dict(chains)
    for a, b in [(127, 129), (129, 127), (1, 2049), (2048, 3), (255, 256)]:
        tc.check_batch(eng, [by_name["chain%d" % a], by_name["chain%d" % b]], want=[0, 0], second_referee=False)
    tc.check_batch(eng, [image for _, image in chains] + [tc.gz(image) for _, image in chains])


def test_gpu_tar_open_walk(eng):
    """shapes of the walk, decoys inside contents, magic, prefix, types and long names: alone, then between
    neighbours, plain and gzipped"""
    cases = tc.doubling_shapes() + tc.decoys() + tc.walk_semantics() + tc.statuses_fine()
    for name, image in cases:
        assert tc.check_batch(eng, [image], want=[0], second_referee=False) == [0], name
    images = [image for _, image in cases]
    images += [tc.gz(image) for image in images if image[:2] != b"\x1f\x8b"]
    assert tc.check_batch(eng, tc.good_images() + images + tc.good_images()) == [0] * (len(images) + 6)
    readers, sts = eng.open_tars([image for _, image in tc.decoys()])
    assert sts == [0, 0, 0]
    assert [[e["path"] for e in r.entries] for r in readers] == [
        [b"inner.tar", b"after"], [b"nines", b"eights", b"e0", b"e1"], [b"inner.tar", b"e0"]]


def test_gpu_tar_open_formats(eng):
    good = tc.good_images()
    assert tc.check_batch(eng, good + [tc.gz(g) for g in good], want=[0] * 6) == [0] * 6


def test_gpu_tar_open_statuses(eng):
    """every status alone between neighbours that open, then all of them in one call"""
    good = tc.good_images()
    cases = tc.statuses()
    for name, image, status in cases:
        assert tc.check_batch(eng, [good[0], image, good[1]], want=[0, status, 0], second_referee=False) == [
            0, status, 0], name
    images, want = [], []
    for name, image, status in cases:
        images += [image, good[2]]
        want += [status, 0]
    tc.check_batch(eng, images, want=want)


def test_gpu_tar_open_precedence(eng):
    good = tc.good_images()
    images, want = [], []
    for name, image, status in tc.precedence():
        assert tc.check_batch(eng, [image, good[2], image], want=[status, 0, status], second_referee=False) == [
            status, 0, status], name
        images.append(image)
        want.append(status)
    tc.check_batch(eng, images, want=want)


def test_gpu_tar_open_plumbing(eng):
    assert eng.open_tars([]) == ([], [])
    good = tc.good_images()
    tc.check_batch(eng, [good[1], good[1], tc.gz(good[1]), tc.gz(good[1])], want=[0] * 4)
    order = list(range(6))
    random.Random(5).shuffle(order)
    tc.check_batch(eng, good + [tc.gz(g) for g in good], close_order=order, second_referee=False)
    tc.check_batch(eng, [b"", b"x", b"\x1f\x8b"], want=[13, 13, 13])


def test_gpu_tar_open_256_mixed(eng):
    images = tc.random_images(20261017, 256, 0.5)
    sts = tc.check_batch(eng, images)
    assert sts.count(0) > 128 and len(set(sts)) >= 4, sorted(set(sts))


def test_gpu_tar_open_libressl(eng):
    """tests/test_tarballs_read.nim's fixture (21 MB, about 41 000 blocks) by itself and in the middle of a batch:
    1743 entries that agree with open_tar field for field"""
    from zippy_amd import api
    fixture = synth.fixture("tarballs/libressl-3.4.2.tar.gz")
    want = tc.alone(eng, fixture)
    assert want[0] == 0 and len(want[2]) == 1743
    good = tc.good_images()
    for images, at in [([fixture], 0), ([good[0], tc.gz(good[1]), fixture, good[2], tc.statuses()[5][1]], 2)]:
        readers, sts = eng.open_tars(images)
        assert sts[at] == 0 and (0, readers[at].data, readers[at].entries) == want
        assert [s != 0 for s in sts] == ([False] if at == 0 else [False] * 4 + [True])  # (the damaged CRC stays alone)
        for r in readers:
            if r is not None:
                r.close()
    readers = api.openTarballs([fixture, good[0]])
    assert len(readers[0].entries) == 1743 and readers[0].contents(5) == want[1][want[2][5]["offset"]:][:want[2][5]["size"]]
    with pytest.raises(api.ZippyError, match="Unexpected EOF"):
        api.openTarballs([good[0], good[0][:700]])
