"""zh_tar_create_batch on a real MI355X (-m gpu): the images of zh_tar_header_kernel against
tests/tar_writer_model.py byte for byte, the .tar.gz against the oracle's compress() of the model's image."""
import gzip
import random

import pytest

import oracle
import synth
import tar_writer_model as twm
from zippy_amd.common import TAR_PLAIN, dfGzip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch  # torch's bundled HIP runtime has to initialise before libzippy_hip.so's
    torch.cuda.init()
    from zippy_amd import api
    e = api.engine()
    e.set_gzip_fname_len(0)
    return e


def _random_entries(rng, n, max_len, pool, prefix="e"):
    out = []
    for i in range(n):
        k = rng.randrange(max_len + 1)
        at = rng.randrange(len(pool) - k + 1)
        kind = "5" if rng.random() < 0.05 else "0"
        out.append(("%s/%d/%s" % (prefix, i % 17, "n%d" % i), (pool[at:at + k], kind, rng.randrange(2 ** 31))))
    return out


def test_gpu_tar_libressl_written_back(eng):
    """tests/test_tarballs_read.nim's fixture (1743 entries, 21 MB): read on the device, written back."""
    reader = eng.open_tar(synth.fixture("tarballs/libressl-3.4.2.tar.gz"))
    entries = [(e["path"], (reader.contents(i), "0", e["mtime"])) for i, e in enumerate(reader.entries)]
    reader.close()
    assert len(entries) == 1743
    img = twm.image(entries)
    assert eng.create_tar(entries, TAR_PLAIN) == img
    gz = eng.create_tar(entries, dfGzip)  # writeTarball's DefaultCompression
    assert gz == oracle.compress(img, -1, oracle.dfGzip, fname_len=0)


@pytest.mark.parametrize("level", [1, -1])
def test_gpu_tar_64mib(eng, level):
    """one image of > 64 MiB: many of deflate.nim:228's 4 MiB blocks in one stream"""
    bufs = synth.gen_batch("mix", 16, 4 << 20)
    entries = [("big/%02d.bin" % i, (bufs[i].tobytes(), "0", 1700000000 + i)) for i in range(16)]
    entries += [("big/tail%d" % k, bytes(range(k % 256)) * 3) for k in range(40)]
    img = twm.image(entries)
    assert len(img) >= 64 << 20
    assert eng.create_tar(entries, TAR_PLAIN) == img
    assert eng.create_tar(entries, dfGzip, level) == oracle.compress(img, level, oracle.dfGzip, fname_len=0)


def test_gpu_tar_256_tarballs_one_call(eng):
    rng = random.Random(20261016)
    pool = synth.gen_batch("mix", 1, 1 << 20)[0].tobytes()
    tars = [_random_entries(rng, rng.randrange(1, 40), rng.choice([0, 600, 5000, 70000]), pool, "t%d" % t)
            for t in range(256)]
    imgs = [twm.image(t) for t in tars]
    outs, sts = eng.create_tars(tars, TAR_PLAIN)
    assert sts == [0] * 256 and outs == imgs
    outs, sts = eng.create_tars(tars, dfGzip, 1)
    assert sts == [0] * 256
    for img, out in zip(imgs, outs):
        assert out == oracle.compress(img, 1, oracle.dfGzip, fname_len=0)


def test_gpu_tar_gzip_first_cap_retry(eng, monkeypatch):
    """ZH_COMPRESS_FIRST_CAP=4096: the larger images of the call outgrow their first slots and are compressed again
    into zh_compress_bound slots, the small ones keep theirs -- the oracle's bytes either way"""
    rng = random.Random(4096)
    pool = synth.gen_batch("mix", 1, 1 << 20)[0].tobytes()
    tars = [_random_entries(rng, rng.randrange(1, 30), rng.choice([0, 600, 70000]), pool, "c%d" % t) for t in range(64)]
    monkeypatch.setenv("ZH_COMPRESS_FIRST_CAP", "4096")
    outs, sts = eng.create_tars(tars, dfGzip, 1)
    assert sts == [0] * 64
    sizes = [len(o) for o in outs]
    assert min(sizes) <= 4096 < max(sizes)
    for t, out in zip(tars, outs):
        assert out == oracle.compress(twm.image(t), 1, oracle.dfGzip, fname_len=0)


def test_gpu_tar_100k_small_entries(eng):
    """headers dominate: 100 000 entries of 0-600 bytes"""
    rng = random.Random(7)
    pool = synth.corpus_file("alice29.txt")
    entries = _random_entries(rng, 100000, 600, pool)
    img = twm.image(entries)
    assert eng.create_tar(entries, TAR_PLAIN) == img
    assert eng.create_tar(entries, dfGzip, 1) == oracle.compress(img, 1, oracle.dfGzip, fname_len=0)


def test_gpu_tar_contract_mode(eng):
    """zh_set_l1_parse(1) at BestSpeed: other bytes than zippy's, the same image inside"""
    rng = random.Random(11)
    pool = synth.gen_batch("mix", 1, 1 << 20)[0].tobytes()
    entries = _random_entries(rng, 300, 20000, pool)
    img = twm.image(entries)
    eng.set_l1_parse(1)
    try:
        gz = eng.create_tar(entries, dfGzip, 1)
    finally:
        eng.set_l1_parse(-1)
    assert oracle.uncompress(gz, oracle.dfGzip) == img
    assert gzip.decompress(gz) == img


def test_gpu_write_tarball_api(eng):
    """zippy_amd.api.writeTarball: an ordered mapping in, the .tar.gz / .tar bytes out, ZippyError on failure"""
    from collections import OrderedDict
    from zippy_amd import api
    from zippy_amd.common import ZippyError
    entries = OrderedDict([("README.txt", (b"Hello, World!", "0", 1600000000)), ("docs", (b"", "5", 0)),
                           ("docs/a.txt", b"a" * 1000)])
    img = twm.image(entries)
    assert api.writeTarball(entries, api.TAR_PLAIN) == img
    assert api.writeTarball(entries) == oracle.compress(img, -1, oracle.dfGzip, fname_len=0)
    with pytest.raises(ZippyError, match="Tarball has no contents"):
        api.writeTarball({})
