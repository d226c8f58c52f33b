"""zh_zip_create_batch on a real MI355X (-m gpu): the archives of zh_zip_create_kernel against
oracle.zip_oracle.create_archive byte for byte."""
import io
import mmap
import random
import zipfile
import zlib

import pytest

import synth
import zip_v2_writer_model as zm
from oracle import zip_oracle
from zippy_amd.common import BestSpeed, ZippyError, to_msdos

pytestmark = pytest.mark.gpu

T, D = to_msdos(1600000000)


@pytest.fixture(scope="module")
def eng():
    import torch  # torch's bundled HIP runtime has to initialise before libzippy_hip.so's
    torch.cuda.init()
    from zippy_amd import api
    return api.engine()


def _random_table(rng, n, max_len, pool, prefix="e"):
    out = []
    for i in range(n):
        k = 0 if rng.random() < 0.05 else rng.randrange(max_len + 1)
        at = rng.randrange(len(pool) - k + 1)
        out.append(("%s/%d/n%d" % (prefix, i % 17, i), pool[at:at + k]))
    return out


def test_gpu_zipc_bagnon_recreated(eng):
    """tests/test_ziparchives_read.nim's fixture: read on the device (zh_zip_open + zh_zip_extract_batch), created
    again as a zip64 archive"""
    reader = eng.open_zip(synth.fixture("ziparchives/Bagnon-10.2.31.zip"))
    files = [i for i, e in enumerate(reader.entries) if not e["is_directory"]]
    outs, sts = reader.extract_batch(files)
    assert sts == [0] * len(files)
    got = dict(zip(files, outs))
    entries = [(e["path"], got.get(i, b"")) for i, e in enumerate(reader.entries)]
    reader.close()
    img = eng.create_zips_one(entries, T, D)
    assert img == zip_oracle.create_archive(entries, T, D)
    with zipfile.ZipFile(io.BytesIO(img)) as zf:
        assert zf.testzip() is None
        assert zf.namelist() == [p for p, _ in reversed(entries)]


def test_gpu_zipc_libressl_entries(eng):
    """tests/test_tarballs_read.nim's fixture: its 1743 entries as one archive"""
    reader = eng.open_tar(synth.fixture("tarballs/libressl-3.4.2.tar.gz"))
    entries = []
    for i, e in enumerate(reader.entries):
        is_dir = e["typeflag"] == b"5"
        entries.append((e["path"] + (b"/" if is_dir and not e["path"].endswith(b"/") else b""), reader.contents(i)))
    reader.close()
    assert len(entries) == 1743
    img = eng.create_zips_one(entries, T, D)
    assert img == zip_oracle.create_archive(entries, T, D)
    assert len(zip_oracle.open_archive(img).records) == 1743


def test_gpu_zipc_256_archives_one_call(eng):
    rng = random.Random(20261016)
    pool = synth.gen_batch("mix", 1, 1 << 20)[0].tobytes()
    tables = [_random_table(rng, rng.randrange(0, 40), rng.choice([0, 600, 5000, 70000]), pool, "z%d" % t)
              for t in range(256)]
    empties = sum(1 for t in tables for _, v in t if not v)
    assert 0.02 < empties / sum(len(t) for t in tables)
    outs, sts = eng.create_zips(tables, T, D)
    assert sts == [0] * 256
    for t, out in zip(tables, outs):
        assert out == zip_oracle.create_archive(t, T, D)
    assert outs == [eng.create_zips_one(t, T, D) for t in tables]  # one archive a call: the same bytes


def test_gpu_zipc_64mib_entry(eng):
    big = synth.gen_batch("mix", 1, 64 << 20)[0].tobytes() + b"tail" * 1001
    entries = [("head.txt", b"small " * 50), ("big/blob.bin", big), ("big/", b"")]
    img = eng.create_zips_one(entries, T, D)
    assert img == zip_oracle.create_archive(entries, T, D)
    with zipfile.ZipFile(io.BytesIO(img)) as zf:
        assert zf.read("big/blob.bin") == big


def test_gpu_zipc_100000_tiny_entries(eng):
    """createZipArchive has no 65535 cap: the count is a zip64 field"""
    entries = [("t/%06d" % i, bytes([i & 255]) * (i % 7)) for i in range(100000)]
    img = eng.create_zips_one(entries, T, D)
    assert img == zip_oracle.create_archive(entries, T, D)
    reader = eng.open_zip(img)
    try:
        assert len(reader.entries) == 100000
        assert reader.entries[0]["path"] == "t/099999" and reader.entries[-1]["path"] == "t/000000"
    finally:
        reader.close()


def test_gpu_zipc_contract_mode(eng):
    """zh_set_l1_parse(1) at BestSpeed: other deflate streams than zippy's around the same framing, valid archives of
    the same contents"""
    rng = random.Random(11)
    pool = synth.gen_batch("mix", 1, 1 << 20)[0].tobytes()
    entries = _random_table(rng, 300, 20000, pool)
    exact = eng.create_zips_one(entries, T, D, BestSpeed)
    eng.set_l1_parse(1)
    try:
        img = eng.create_zips_one(entries, T, D, BestSpeed)
    finally:
        eng.set_l1_parse(-1)
    assert exact == zip_oracle.create_archive(entries, T, D)
    (frame, streams), (frame_exact, streams_exact) = zm.framing(img), zm.framing(exact)
    assert frame == frame_exact and len(streams) == len(streams_exact) == 300
    assert streams != streams_exact
    r = zip_oracle.open_archive(img)
    with zipfile.ZipFile(io.BytesIO(img)) as zf:
        assert zf.testzip() is None
        for p, v in entries:
            assert zf.read(p) == v == zip_oracle.extract_file(r, p)


@pytest.mark.timeout(3000)
def test_gpu_zipc_entry_beyond_4gib(eng):
    """one entry of 2^32 + 12345 bytes, from an anonymous mapping: legal in a zip64 archive.  No oracle call (the
    Python oracle would copy 4 GiB several times): zipfile reads the length back, and the CRC-32 is zlib's"""
    n = (1 << 32) + 12345
    mm = mmap.mmap(-1, n, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS)
    try:
        mm[0:5] = b"first"
        mm[(1 << 32) - 3:(1 << 32) + 3] = b"border"
        mm[n - 4:n] = b"last"
        outs, sts = eng.create_zips([[("huge.bin", mm)], [("ok.txt", b"fine")]], T, D)
        assert sts == [0, 0]
        assert outs[1] == zip_oracle.create_archive([("ok.txt", b"fine")], T, D)
        crc, view = 0, memoryview(mm)
        for at in range(0, n, 1 << 26):
            crc = zlib.crc32(view[at:at + (1 << 26)], crc)
        view.release()
        with zipfile.ZipFile(io.BytesIO(outs[0])) as zf:
            info = zf.infolist()[0]
            assert (info.filename, info.file_size, info.CRC) == ("huge.bin", n, crc)
            assert info.compress_size == len(outs[0]) - (30 + 8 + 20) - (46 + 8 + 28) - 98
            with zf.open(info) as f:  # the stream itself: decoded in pieces, compared with the mapping
                at = 0
                while True:
                    piece = f.read(1 << 24)
                    if not piece:
                        break
                    assert piece == mm[at:at + len(piece)]
                    at += len(piece)
                assert at == n
    finally:
        import gc
        gc.collect()
        mm.close()


def test_gpu_create_zip_archives_api(eng):
    """zippy_amd.api.createZipArchives: ordered mappings in, the archives' bytes out, ZippyError on the first failure"""
    from collections import OrderedDict
    from zippy_amd import api
    tables = [OrderedDict([("README.txt", b"Hello, World!"), ("docs/", b""), ("docs/a.txt", b"a" * 1000)]),
              OrderedDict(), [("b.bin", bytes(range(256)) * 9)]]
    assert api.createZipArchives(tables, T, D) == [zip_oracle.create_archive(t, T, D) for t in tables]
    assert api.createZipArchives(tables, T, D, 9) == [zm.image(t, T, D, 9) for t in tables]
    assert api.createZipArchives(tables[:1], T, D) == [api.createZipArchive(tables[0], T, D)]
    assert api.createZipArchives([]) == []
    with pytest.raises(ZippyError, match="Invalid file name"):
        api.createZipArchives([tables[0], {"/abs": b"x"}])
    assert BestSpeed == 1
