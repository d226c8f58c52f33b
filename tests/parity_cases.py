"""Parity cases shared by tests/test_gpu_parity.py (real MI355X through
zippy_amd/libzippy_hip.so) and tests/test_emu_parity.py (the same kernel sources
under the CPU emulator).  `eng` is a zippy_amd._binding.Engine; the oracle
(oracle/) is the checker.  Mirrors the reference's own tests."""
import hashlib
import heapq
import os
import random
import struct
import zlib

import numpy as np

import deflate_craft as dc
import oracle
import synth

WBITS = {oracle.dfDeflate: -15, oracle.dfZlib: 15, oracle.dfGzip: 31}
FORMATS = (oracle.dfDeflate, oracle.dfZlib, oracle.dfGzip)


def check_fixtures(eng, max_len=None):
    """tests/test.nim:41-60, tests/test_known_bad.nim:3 -- bit-exact decode."""
    names, blobs = [], []
    for name, meta in synth.manifest()["fixtures"].items():
        if max_len is None or meta["len"] <= max_len:
            names.append(name)
            blobs.append(synth.fixture(name))
    outs, sts = eng.uncompress_batch(blobs)
    for name, out, st in zip(names, outs, sts):
        meta = synth.manifest()["fixtures"][name]
        assert st == 0, (name, st)
        assert len(out) == meta["len"], name
        assert hashlib.sha256(out).hexdigest() == meta["sha256"], name


def check_compress_identical(eng, inputs, levels, formats=FORMATS):
    """Device output == oracle output, byte for byte; an independent decoder
    (zlib) and the oracle's zippy-equivalent decoder both round-trip it."""
    eng.set_gzip_fname_len(0)
    for level in levels:
        for fmt in formats:
            outs, sts = eng.compress_batch(inputs, level, fmt)
            for src, out, st in zip(inputs, outs, sts):
                assert st == 0, (level, fmt, len(src), st)
                ref = oracle.compress(src, level, fmt, fname_len=0)
                assert out == ref, "level %d fmt %d len %d: device %d B vs oracle %d B" % (
                    level, fmt, len(src), len(out), len(ref))
                assert zlib.decompress(out, WBITS[fmt]) == src
                assert oracle.uncompress(out, fmt) == src


def check_parallel_parse(eng, inputs, formats=(oracle.dfGzip,), margin=1.02):
    """The opt-in parallel BestSpeed parse (zh_set_l1_parse(ctx, 1), csrc/zh_l1p_match.hip) under the
    encoder contract of BASELINE.json's north star: every stream decodes to its input through the
    oracle's zippy-equivalent uncompress AND through zlib, the streams of a batch are together no
    larger than `margin` x the oracle's (= zippy's) at level 1, the result does not depend on the
    run, and the other levels still give the oracle's bytes while the switch is on."""
    eng.set_gzip_fname_len(0)
    eng.set_l1_parse(1)
    try:
        for fmt in formats:
            outs, sts = eng.compress_batch(inputs, 1, fmt)
            again, _ = eng.compress_batch(inputs, 1, fmt)
            dev = ref = 0
            for src, out, st in zip(inputs, outs, sts):
                assert st == 0, (fmt, len(src), st)
                assert zlib.decompress(out, WBITS[fmt]) == src, (fmt, len(src))
                assert oracle.uncompress(out, fmt) == src, (fmt, len(src))
                dev += len(out)
                ref += len(oracle.compress(src, 1, fmt, fname_len=0))
            assert outs == again, "parallel parse: two runs, two results"
            assert dev <= margin * ref, "parallel parse: %d B against the oracle's %d B" % (dev, ref)
            back, sts2 = eng.uncompress_batch(outs, oracle.dfDeflate if fmt == oracle.dfDeflate
                                              else oracle.dfDetect)
            assert all(x == 0 for x in sts2) and back == list(inputs)
        small = [b for b in inputs if len(b) <= 70000][:6]
        for level in (-2, 0, -1):
            outs, sts = eng.compress_batch(small, level, oracle.dfGzip)
            for src, out in zip(small, outs):
                assert out == oracle.compress(src, level, oracle.dfGzip, fname_len=0), level
    finally:
        eng.set_l1_parse(-1)
    return dev, ref


def huffman_histograms():
    """Histograms for the code builders: random and skewed ones, Fibonacci frequencies (a tree deeper than any
    limit), one / two / no symbols used, equal frequencies (ties everywhere), the three alphabets' sizes."""
    rnd = random.Random(31)
    out = []
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    for n, minc, limit in ((286, 257, 15), (30, 2, 15), (19, 19, 7)):
        out.append((np.zeros(n, np.uint32), minc, limit))
        for k in (0, 3, n - 1):
            f = np.zeros(n, np.uint32)
            f[k] = 5
            out.append((f, minc, limit))
        f = np.zeros(n, np.uint32)
        f[1] = f[n - 2] = 7
        out.append((f, minc, limit))
        out.append((np.full(n, 3, np.uint32), minc, limit))
        out.append((np.arange(1, n + 1, dtype=np.uint32), minc, limit))
        m = min(n, 34)
        f = np.zeros(n, np.uint32)
        order = list(range(n))
        rnd.shuffle(order)
        for i in range(m):
            f[order[i]] = fib[i]
        out.append((f, minc, limit))
        for _ in range(12):
            used = rnd.randrange(2, n + 1)
            f = np.zeros(n, np.uint32)
            for i in rnd.sample(range(n), used):
                f[i] = max(1, int(rnd.expovariate(1.0 / rnd.choice((2, 50, 5000, 400000)))))
            out.append((f, minc, limit))
    return out


def check_huffman_builders(eng):
    """zh_debug_huffman: the byte-identical builder gives the oracle's huffmanCodes symbol for symbol (codes and
    lengths); contract mode's gives a complete prefix code within the limit whose payload is the optimum's where
    no length had to be cut (= the oracle's cost there) and within 1 % + 16 bits of the oracle's where some had."""
    for f, minc, limit in huffman_histograms():
        want_codes, want_lens = oracle.huffman_codes(f, minc, limit)
        codes, lens = eng.debug_huffman(f, minc, limit, contract=False)
        assert list(lens) == list(want_lens) and list(codes) == list(want_codes), (len(f), limit, "exact builder")
        codes, lens = eng.debug_huffman(f, minc, limit, contract=True)
        assert len(lens) == len(want_lens), (len(f), limit)
        used = [i for i in range(len(f)) if f[i]]
        if len(used) >= 2:
            assert all(1 <= lens[i] <= limit for i in used) and all(lens[i] == 0 for i in range(len(lens)) if i >= len(f) or not f[i])
            assert sum(2.0 ** -int(lens[i]) for i in used) == 1.0, "not a complete prefix code"
            seen = set()
            for i in used:  # canonical, bit-reversed: no code is another's prefix (read first bit first)
                bits = format(int(codes[i]), "0%db" % lens[i])[::-1]
                assert all(bits[:k] not in seen for k in range(1, len(bits) + 1)), "prefix clash"
                seen.add(bits)
            cost = sum(int(f[i]) * int(lens[i]) for i in used)
            ref = sum(int(f[i]) * int(want_lens[i]) for i in used)
            unlimited = _huffman_cost(f)
            if max(int(lens[i]) for i in used) < limit and max(int(want_lens[i]) for i in used) < limit:
                assert cost == unlimited == ref, (cost, unlimited, ref)
            else:
                assert unlimited <= cost <= ref * 1.01 + 16, (cost, ref, unlimited)
        else:
            assert list(lens) == list(want_lens), "special cases as deflate.nim:34-45"


def _huffman_cost(f):
    import heapq
    h = [int(x) for x in f if x]
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        cost += a + b
        heapq.heappush(h, a + b)
    return cost


def wide_length_count_input():
    """deflate.nim:136-139 counts the symbols of a code length in a uint8, which
    wraps when 256 or more share one length.  3000 bytes at level -2 (Huffman only, no stored
    fallback, dynamic codes because the block is longer than 2048 bytes): one byte value 2745
    times, the other 255 values once each -- with the end-of-block symbol that is 256 symbols of
    frequency 1 under one subtree: 256 codes of length 9."""
    rnd = random.Random(95)
    body = [0x41] * 2745 + [v for v in range(256) if v != 0x41]
    rnd.shuffle(body)
    return bytes(body)


def check_wide_code_length_counts(eng):
    """The case of SURVEY.md 9.5 through device, oracle and zlib: oracle and kernel count in wide
    integers on purpose (the reference's wrap would emit a stream that does not decode)."""
    import heapq
    src = wide_length_count_input()
    # the premise, worked out independently: Huffman code lengths of the literal/length alphabet
    freq = [0] * 286
    for b in src:
        freq[b] += 1
    freq[256] = 1
    heap = [(f, i, None, None) for i, f in enumerate(freq) if f]
    heapq.heapify(heap)
    n = 286
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], n, a, b))
        n += 1
    depth = {}

    def walk(node, d):
        if node[2] is None:
            depth[node[1]] = d
        else:
            walk(node[2], d + 1)
            walk(node[3], d + 1)
    walk(heap[0], 0)
    per_len = {}
    for d in depth.values():
        per_len[d] = per_len.get(d, 0) + 1
    assert max(per_len.values()) >= 256, per_len
    eng.set_gzip_fname_len(0)
    for fmt in (oracle.dfGzip, oracle.dfDeflate):
        out = eng.compress(src, -2, fmt)
        assert out == oracle.compress(src, -2, fmt, fname_len=0)
        assert zlib.decompress(out, WBITS[fmt]) == src
        assert oracle.uncompress(out, fmt) == src
        assert eng.uncompress(out, fmt) == src


def check_roundtrip(eng, inputs, level, fmt=oracle.dfGzip):
    outs, sts = eng.compress_batch(inputs, level, fmt)
    assert all(s == 0 for s in sts)
    back, sts2 = eng.uncompress_batch(outs, oracle.dfDeflate if fmt == oracle.dfDeflate
                                      else oracle.dfDetect)
    assert all(s == 0 for s in sts2), sts2
    for src, b in zip(inputs, back):
        assert b == src


def check_tokens(eng, src, level):
    """Device match list re-expressed as the reference's u16 token stream
     == oracle token stream, block by block."""
    dev = eng.debug_tokens(src, level)
    parts = [oracle.block_tokens(src, level, o, min(len(src) - o, 4194304))[0]
             for o in range(0, max(len(src), 1), 4194304)]
    want = np.concatenate(parts) if parts else np.zeros(0, np.uint16)
    assert np.array_equal(dev, want), (level, len(dev), len(want))


def check_gzip_random_fname(eng, src):
    """zippy.nim:26-42: FNAME of 0..25 letters chosen per call."""
    eng.set_gzip_fname_len(-1)
    seen = set()
    for _ in range(12):
        out = eng.compress(src, 1, oracle.dfGzip)
        assert out[:4] == b"\x1f\x8b\x08\x08"
        k = out.index(b"\x00", 10) - 10
        assert 0 <= k <= 25 and out[10:10 + k] == bytes(range(97, 97 + k))
        seen.add(k)
        assert zlib.decompress(out, 31) == src
        assert oracle.uncompress(out) == src
    eng.set_gzip_fname_len(0)
    assert len(seen) > 1


def check_checksums(eng, blobs):
    for d in blobs:
        assert eng.crc32(d) == zlib.crc32(d)
        assert eng.adler32(d) == zlib.adler32(d)


def check_errors_match_oracle(eng, blobs, data_format=oracle.dfDetect):
    """tests/fuzz.nim / tests/stress.nim contract: a damaged stream either fails
    (any ZippyError) or decodes; device and oracle must agree on which, and on
    the bytes when it decodes."""
    outs, sts = eng.uncompress_batch(blobs, data_format)
    for blob, out, st in zip(blobs, outs, sts):
        try:
            want = oracle.uncompress(blob, data_format)
            ok = True
        except oracle.ZippyError:
            ok = False
        assert (st == 0) == ok, (len(blob), st, ok)
        if ok:
            assert out == want


def mutated_fixtures(count, seed, max_len=70000):
    """tests/fuzz.nim:16-33: flip one byte, then truncate at that position."""
    files = ["randtest1.gz", "randtest2.gz", "randtest3.gz", "rfctest1.gz", "rfctest2.gz",
             "rfctest3.gz", "zerotest1.gz", "zerotest2.gz"]
    files = [f for f in files if synth.manifest()["fixtures"][f]["len"] <= max_len]
    rng = random.Random(seed)
    blobs = []
    for _ in range(count):
        comp = bytearray(synth.fixture(rng.choice(files)))
        pos = rng.randrange(len(comp))
        comp[pos] = rng.randrange(256)
        blobs.append(bytes(comp))
        blobs.append(bytes(comp[:pos]))
    return blobs


def edge_inputs():
    rnd = random.Random(5)
    text = synth.corpus_file("alice29.txt")
    sizes = [0, 1, 2, 4, 5, 14, 15, 16, 17, 255, 256, 2047, 2048, 2049, 32767, 32768, 32769,
             65535, 65536, 65537]
    out = [text[:n] for n in sizes]
    out += [bytes(range(256)), b"\x00" * 70000, rnd.randbytes(70000), b"ab" * 20000]
    return out


def check_error_statuses(eng):
    gz = bytearray(oracle.compress(b"hello world" * 10, 1, fname_len=0))

    def status_of(blob, fmt=oracle.dfDetect):
        _, sts = eng.uncompress_batch([bytes(blob)], fmt)
        return sts[0]

    bad = bytearray(gz)
    bad[3] |= 4
    assert status_of(bad) == 12  # FEXTRA, gzip.nim:40-41
    bad = bytearray(gz)
    bad[-5] ^= 1
    assert status_of(bad) == 8  # CRC, gzip.nim:80-81
    bad = bytearray(gz)
    bad[-1] ^= 1
    assert status_of(bad) != 0  # ISIZE, gzip.nim:83-88
    assert status_of(b"\x00" * 30) == 3  # detect, zippy.nim:125
    assert status_of(b"\x07" + b"\x00" * 16, oracle.dfDeflate) == 17  # BTYPE 3, inflate.nim:288
    # a bad stream must not poison its neighbours
    good = oracle.compress(b"neighbour" * 100, 1, fname_len=0)
    outs, sts = eng.uncompress_batch([good, bytes(bad), good])
    assert sts[0] == 0 and sts[2] == 0 and sts[1] != 0
    assert outs[0] == b"neighbour" * 100 and outs[2] == outs[0]
    # A gzip member whose ISIZE (the host path's output capacity) is far below what its body
    # produces -- one stored block of 65535 bytes behind ISIZE = 1, and a literal/match body
    # behind ISIZE = 3: the decoder stops at the capacity, and the checksum pass must not read
    # past the slot (it did once: out_len overshot the slot by the failing token).  The oracle
    # decodes with a growing buffer and then fails on the size/CRC check; both must reject.
    import struct
    big = bytes(range(256)) * 256
    stored = b"\x01" + struct.pack("<HH", 65535, 0) + big[:65535]
    liar = b"\x1f\x8b\x08\x00" + b"\x00" * 6 + stored + struct.pack("<II", zlib.crc32(big[:65535]), 1)
    assert status_of(liar) != 0
    body = zlib.compress(b"abcdefgh" * 4000, 6)[2:-4]
    liar2 = b"\x1f\x8b\x08\x00" + b"\x00" * 6 + body + struct.pack("<II", 0, 3)
    assert status_of(liar2) != 0
    for blob in (liar, liar2):
        try:
            oracle.uncompress(blob)
            assert False, "the oracle must reject it too"
        except oracle.ZippyError:
            pass
    outs, sts = eng.uncompress_batch([good, liar, liar2, good])
    assert sts[0] == 0 and sts[3] == 0 and sts[1] != 0 and sts[2] != 0 and outs[3] == outs[0]
    import pytest
    from zippy_amd.common import ZippyError
    for level in (10, -3):
        with pytest.raises(ZippyError):
            eng.compress(b"x", level)
    with pytest.raises(ZippyError):
        eng.compress(b"x", 1, oracle.dfDetect)


def check_blocks(eng, src, levels, block_sizes, formats=(oracle.dfGzip,)):
    """Block-parallel form (BASELINE config 5): bytes and index equal the oracle's at the same block
    size, the stream round-trips through the oracle's plain uncompress() and zlib, and the indexed
    decode returns the input."""
    import zlib
    for level in levels:
        for bb in block_sizes:
            for fmt in formats:
                want, want_idx = oracle.compress_blocks(src, level, fmt, bb, fname_len=0)
                got, idx = eng.compress_blocks(src, level, fmt, bb)
                assert got == want, "level %d block %d fmt %d: bytes differ" % (level, bb, fmt)
                assert idx == want_idx, "level %d block %d fmt %d: index differs" % (level, bb, fmt)
                assert oracle.uncompress(got, fmt) == src
                wbits = {oracle.dfGzip: 31, oracle.dfZlib: 15, oracle.dfDeflate: -15}[fmt]
                assert zlib.decompress(got, wbits) == src
                assert eng.uncompress_indexed(got, idx, fmt) == src
                assert eng.uncompress(got, fmt) == src
                if bb == 4194304:
                    assert got == oracle.compress(src, level, fmt, fname_len=0)


def check_blocks_bad_index(eng, src):
    """An index that does not describe the stream fails the call instead of returning wrong bytes."""
    import pytest
    from zippy_amd.common import ZippyError
    got, idx = eng.compress_blocks(src, 1, oracle.dfGzip, 32768)
    assert len(idx) >= 4
    for bad in (
        [idx[0], (idx[1][0] + 1, idx[1][1])] + idx[2:],          # block 1 starts one bit late
        [idx[0], (idx[1][0], idx[1][1] - 7)] + idx[2:],          # block 0 promises 7 bytes less
        idx[:-1] + [(idx[-1][0], idx[-1][1] + 1)],               # total one byte too long
        [idx[0], idx[2]] + idx[2:],                              # repeated entry: block skipped
    ):
        with pytest.raises(ZippyError):
            eng.uncompress_indexed(got, bad, oracle.dfGzip)
    damaged = bytearray(got)
    damaged[len(damaged) // 2] ^= 0x10
    with pytest.raises(ZippyError):
        eng.uncompress_indexed(bytes(damaged), idx, oracle.dfGzip)


# ---- ZIP archives (reference tests: tests/test_ziparchives_read.nim,
# tests/test_ziparchives_write.nim) ----
ZIP_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ziparchives")


def zip_fixture(name):
    with open(os.path.join(ZIP_DIR, name), "rb") as fh:
        return fh.read()


def check_zip_extract(eng, image):
    """Every record of the archive, extracted in one batch, equals the oracle's extractFile."""
    from oracle import zip_oracle
    want = zip_oracle.open_archive(image)
    reader = eng.open_zip(image)
    assert [e["path"].encode("utf-8", "surrogateescape") for e in reader.entries] == list(want.records)
    for e in reader.entries:
        w = want.records[e["path"].encode("utf-8", "surrogateescape")]
        for key in ("is_directory", "header_offset", "crc32", "compressed_size", "uncompressed_size", "unix_mode"):
            assert e[key] == w[key], (e["path"], key)
    files = [i for i, e in enumerate(reader.entries) if not e["is_directory"]]
    outs, sts = reader.extract_batch(files)
    assert all(s == 0 for s in sts)
    for i, out in zip(files, outs):
        assert out == zip_oracle.extract_file(want, reader.entries[i]["path"]), reader.entries[i]["path"]
    dirs = [i for i, e in enumerate(reader.entries) if e["is_directory"]]
    if dirs:
        _, sts = reader.extract_batch(dirs[:3])
        assert all(s == 26 for s in sts)  # "No file record found", ziparchives.nim:89-90
    assert reader.walk_files() == [p.decode("utf-8", "surrogateescape") for p, r in want.records.items()
                                   if not r["is_directory"]]
    reader.close()
    return len(files)


def check_zip_create(eng, entries, dos_time=0x6000, dos_date=0x5a21):
    """createZipArchive: same bytes as the oracle, readable by Python's zipfile, and back."""
    import io
    import zipfile
    from oracle import zip_oracle
    got = eng.create_zip(entries, dos_time, dos_date)
    assert got == zip_oracle.create_archive(entries, dos_time, dos_date)
    zf = zipfile.ZipFile(io.BytesIO(got))
    assert zf.testzip() is None
    pairs = list(entries.items()) if hasattr(entries, "items") else list(entries)
    assert zf.namelist() == [p for p, _ in reversed(pairs)]
    for path, contents in pairs:
        assert zf.read(path) == bytes(contents)
    reader = eng.open_zip(got)
    outs, sts = reader.extract_batch(list(range(len(pairs))))
    assert all(s == 0 for s in sts)
    assert outs == [bytes(c) for _, c in reversed(pairs)]
    reader.close()
    return got


def check_zip_errors(eng):
    import pytest
    from zippy_amd.common import ZippyError
    from oracle import zip_oracle
    either = (ZippyError, oracle.ZippyError)
    good = eng.create_zip([("a.txt", b"hello " * 50), ("dir/b.bin", bytes(range(256)) * 8), ("empty", b"")])
    # damaged payload -> that record fails its CRC (or decode), neighbours survive
    bad = bytearray(good)
    reader = eng.open_zip(good)
    target = reader.entries[1]  # "dir/b.bin"... entries are listed last to first
    reader.close()
    bad[target["header_offset"] + 30 + len(target["path"]) + 20 + 5] ^= 0x40
    reader = eng.open_zip(bytes(bad))
    outs, sts = reader.extract_batch([0, 1, 2])
    assert sts[1] != 0 and sts[0] == 0 and sts[2] == 0
    with pytest.raises(either):
        zip_oracle.extract_file(zip_oracle.open_archive(bytes(bad)), target["path"])
    reader.close()
    for blob in (b"", b"PK\x05\x06", good[:-30], good[:len(good) // 2]):
        with pytest.raises(ZippyError):
            eng.open_zip(blob)
        with pytest.raises(either):
            zip_oracle.open_archive(blob)
    # zip64 fields near INT64_MAX / above it (an overflow-checked reference raises; here the
    # bounds checks must not wrap): a zip64 locator pointing its EOCD64 at 0x7fffffffffffffe0,
    # and a real EOCD64 whose directory offset / size / record count are absurd
    import struct
    eocd = b"PK\x05\x06" + b"\x00" * 18
    for off in (0x7fffffffffffffe0, 0xffffffffffffffff, 1 << 63, 1 << 40):
        blob = b"PK\x06\x07" + struct.pack("<IQI", 0, off, 1) + eocd
        with pytest.raises(ZippyError):
            eng.open_zip(blob)
    for fields in ((1, 1, 0x7ffffffffffffff0, 0), (1, 1, 0, 0x7ffffffffffffff0), (1 << 62, 1 << 62, 10, 0),
                   (0xffffffffffffffff, 0xffffffffffffffff, 46, 0)):
        e64 = b"PK\x06\x06" + struct.pack("<QHHIIQQQQ", 44, 45, 45, 0, 0, *fields)
        blob = e64 + b"PK\x06\x07" + struct.pack("<IQI", 0, 0, 1) + eocd
        with pytest.raises(ZippyError):
            eng.open_zip(blob)
    for entries in ([("", b"x")], [("/abs", b"x")], [("n" * 70000, b"x")]):
        with pytest.raises(ZippyError):
            eng.create_zip(entries)
        with pytest.raises(either):
            zip_oracle.create_archive(entries)
    with pytest.raises(ZippyError):
        eng.open_zip(good).extract_file("nope.txt")


# ---- tarballs (reference test: tests/test_tarballs_read.nim) ----
def tar_fixture():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tarballs",
                           "libressl-3.4.2.tar.gz"), "rb") as fh:
        return fh.read()


def check_tarball(eng, image):
    from oracle import tar_oracle
    data, want = tar_oracle.open_tarball(image)
    reader = eng.open_tar(image)
    assert reader.data == data
    assert reader.entries == want
    reader.close()
    return len(want)


def make_tar_gz(files, long_name=None):
    """A small .tar.gz with Python's tarfile (GNU format: a long name becomes an 'L' block)."""
    import io
    import tarfile
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w:gz", format=tarfile.GNU_FORMAT) as tf:
        for name, contents in files:
            if contents is None:
                info = tarfile.TarInfo(name)
                info.type = tarfile.DIRTYPE
                info.mode = 0o755
                tf.addfile(info)
            else:
                info = tarfile.TarInfo(name)
                info.size = len(contents)
                info.mode = 0o644
                info.mtime = 1234567890
                tf.addfile(info, io.BytesIO(contents))
        if long_name:
            info = tarfile.TarInfo(long_name)
            info.size = 3
            tf.addfile(info, io.BytesIO(b"abc"))
        link = tarfile.TarInfo("link")
        link.type = tarfile.SYMTYPE
        link.linkname = "a.txt"
        tf.addfile(link)
    return buf.getvalue()


def check_tar_errors(eng):
    import gzip
    import pytest
    from zippy_amd.common import ZippyError
    from oracle import tar_oracle
    either = (ZippyError, oracle.ZippyError)
    good = gzip.decompress(make_tar_gz([("a.txt", b"hello")]))
    for bad in (good[:515],                                        # cut inside the first file
                good[:156] + b"Z" + good[157:],                    # vendor type: skipped, not an error
                good[:156] + b"7" + good[157:],                    # unsupported type
                b"../evil".ljust(100, b"\0") + good[100:],         # unsafe path
                good[:124] + b"0000000009\0" + good[135:]):        # "9" is not octal
        expect_ok = bad[156:157] == b"Z"
        for fn in (lambda b: eng.open_tar(b), tar_oracle.open_tarball):
            if expect_ok:
                fn(bad)
            else:
                with pytest.raises(either):
                    fn(bad)
    with pytest.raises(either):
        eng.open_tar(b"\x1f\x8b" + b"\0" * 30)


def check_ragged_staging(eng, scale):
    """Host-buffer calls whose buffers straddle the staging chunks (upload) and whose results
    straddle them again (download): ragged sizes, empty buffers in between, one buffer of
    several chunks.  `scale` stretches the sizes (1 for the emulator's 128 KiB chunks)."""
    import synth
    sizes = [0, 70001, 1, 262144 + 13, 0, 0, 4095, 400000 + 7, 65536, 131072, 3, 0, 99999, 0]
    pool = synth.gen_batch("mix", 8, 1 << 20).tobytes()
    bufs, at = [], 0
    for k, sz in enumerate(sizes):
        sz *= scale
        rep = -(-(sz + 1) // len(pool))
        bufs.append((pool * rep)[at % 4096:at % 4096 + sz])
        at += 977
    for level, fmt in ((1, oracle.dfGzip), (0, oracle.dfZlib), (-2, oracle.dfDeflate)):
        # one plan for the whole batch, then the same batch as pipelined groups: identical results
        try:
            eng.set_host_pipeline(1 << 60, 0)
            outs, sts = eng.compress_batch(bufs, level, fmt)
            eng.set_host_pipeline(1, 150000 * scale)
            outs2, sts2 = eng.compress_batch(bufs, level, fmt)
        finally:
            eng.set_host_pipeline(0, 0)
        assert all(s == 0 for s in sts), sts
        assert sts2 == sts and outs2 == outs, level
        for i in (1, 3, 7, 12) if scale > 1 else range(len(bufs)):
            assert outs[i] == oracle.compress(bufs[i], level, fmt, fname_len=0), (level, i)
        back, sts = eng.uncompress_batch(outs, fmt)
        assert all(s == 0 for s in sts), sts
        assert back == bufs, level
        if fmt == oracle.dfGzip:
            # the same batch as pipelined groups (batch_pipelined: gzip members carry their
            # size): identical results; then one member whose ISIZE promises too little -- the group it
            # is in outgrows its slot and the whole batch is sent down the plain path, which sizes and
            # retries: same bytes, that member's status from the ISIZE check like the plain path's
            try:
                eng.set_host_pipeline(1, 150000 * scale)
                back2, sts2 = eng.uncompress_batch(outs, fmt)
                liar = list(outs)
                k = 7
                small = (len(bufs[k]) // 2).to_bytes(4, "little")
                liar[k] = liar[k][:-4] + small
                back3, sts3 = eng.uncompress_batch(liar, fmt)
                bad7 = list(outs)
                bad7[k] = bad7[k][:len(bad7[k]) // 2] + bytes([bad7[k][len(bad7[k]) // 2] ^ 0x55]) + bad7[k][len(bad7[k]) // 2 + 1:]
                back4, sts4 = eng.uncompress_batch(bad7, fmt)
            finally:
                eng.set_host_pipeline(1 << 60, 0)
            assert sts2 == sts and back2 == back, "pipelined uncompress differs"
            plain3, psts3 = eng.uncompress_batch(liar, fmt)
            plain4, psts4 = eng.uncompress_batch(bad7, fmt)
            eng.set_host_pipeline(0, 0)
            assert sts3 == psts3 and back3 == plain3 and sts3[k] != 0, (sts3, psts3)
            assert sts4 == psts4 and back4 == plain4 and sts4[k] != 0
            assert [b for i, b in enumerate(back3) if i != k] == [b for i, b in enumerate(bufs) if i != k]
        if fmt == oracle.dfGzip:  # a damaged member in the middle only fails its own slot
            bad = list(outs)
            bad[7] = bad[7][:len(bad[7]) // 2] + bytes([bad[7][len(bad[7]) // 2] ^ 0x55]) + bad[7][len(bad[7]) // 2 + 1:]
            back, sts = eng.uncompress_batch(bad, fmt)
            assert sts[7] != 0 and back[7] is None
            assert [b for i, b in enumerate(back) if i != 7] == [b for i, b in enumerate(bufs) if i != 7]


def check_batch_into(eng):
    """zh_compress_batch_into / zh_uncompress_batch_into: the results of the ordinary calls, in
    buffers of the caller's; one that is too small only fails its own slot -- with ZH_ERR_DST_TOO_SMALL,
    which is what a binding grows and retries on (include/zippy_hip.h) -- and learns its size.  Once as
    one plan, once as pipelined groups."""
    import synth
    TOO_SMALL = 21  # ZH_ERR_DST_TOO_SMALL
    eng.set_gzip_fname_len(0)
    bufs = [b.tobytes() for b in synth.gen_batch("mix", 5, 70001)] + [b"", b"x" * 300, synth.corpus_file("html")]
    want, sts = eng.compress_batch(bufs, 1, oracle.dfGzip)
    for pipe in ((1 << 60, 0), (1, 150000)):
        try:
            eng.set_host_pipeline(*pipe)
            outs = [bytearray(eng.compress_bound(len(b))) for b in bufs]
            outs[2] = bytearray(100)  # too small
            lens, sts2, filled = eng.compress_batch_into(bufs, outs, 1, oracle.dfGzip)
            for i, b in enumerate(bufs):
                assert lens[i] == len(want[i]), (pipe, i)
                if i == 2:
                    assert sts2[i] == TOO_SMALL and not filled[i], (pipe, sts2[i])
                else:
                    assert sts2[i] == 0 and filled[i] and bytes(outs[i][:lens[i]]) == want[i], (pipe, i)
            for fmt in (oracle.dfGzip, oracle.dfZlib, oracle.dfDeflate):
                blobs, _ = eng.compress_batch(bufs, 1, fmt)
                back = [bytearray(len(b)) for b in bufs]
                back[4] = bytearray(len(bufs[4]) - 1)  # one byte short
                back[7] = bytearray(5)                 # far too short (a sized stream takes the sizing pass)
                blobs = list(blobs)
                blobs[1] = blobs[1][:len(blobs[1]) // 2]  # and a damaged stream
                lens, sts3, filled = eng.uncompress_batch_into(blobs, back, fmt)
                for i, b in enumerate(bufs):
                    if i == 1:
                        assert sts3[i] not in (0, TOO_SMALL), (pipe, fmt, sts3[i])
                    elif i in (4, 7):
                        assert sts3[i] == TOO_SMALL and lens[i] == len(b) and not filled[i], (pipe, fmt, i, sts3[i], lens[i])
                    else:
                        assert sts3[i] == 0 and filled[i] and lens[i] == len(b) and bytes(back[i]) == b, (pipe, fmt, i)
        finally:
            eng.set_host_pipeline(0, 0)


def check_unsized_streams(eng):
    """zlib / raw deflate streams carry no size: the host call guesses 4x, and streams that
    outgrow the guess are sized and decoded again -- next to streams that fit, damaged ones and
    (for dfDetect) gzip members, in one call."""
    import zlib
    import synth
    text = synth.corpus_file("alice29.txt")[:90000]
    rnd = np.random.default_rng(11).integers(0, 256, 140001, dtype=np.uint8).tobytes()
    plain = [b"", b"a", text, b"\x00" * 300000, bytes(range(256)) * 40, b"ab" * 70000, text[:777],
             b"\xff" * 1000000,
             # (round 6: the sizing pass runs on the tokens kernel's count-only form) markup that compresses 6-7 x in many
             # dynamic blocks (system zlib's); three stored blocks and then a long run: stored chains and codes in one sized stream
             rnd + b"\x07" * 2000003,
             synth.corpus_file("html_x_4") + synth.corpus_file("html_x_4")[:190001]]
    for fmt, wb in ((oracle.dfZlib, 15), (oracle.dfDeflate, -15)):
        blobs = []
        for k, b in enumerate(plain):
            if k % 2:
                c = zlib.compressobj(6, zlib.DEFLATED, wb)
                blobs.append(c.compress(b) + c.flush())
            else:
                blobs.append(oracle.compress(b, 1, fmt))
        hurt = bytearray(blobs[3])
        hurt[len(hurt) // 2] ^= 0x40
        blobs.append(bytes(hurt))           # damaged, highly compressible
        blobs.append(blobs[2][:len(blobs[2]) // 2])  # truncated
        outs, sts = eng.uncompress_batch(blobs, fmt)
        for i, blob in enumerate(blobs):
            try:
                want = oracle.uncompress(blob, fmt)
            except oracle.ZippyError:
                want = None
            assert (outs[i] if sts[i] == 0 else None) == want, (fmt, i, sts[i])
            if i < len(plain):
                assert want == plain[i]
    mixed = [oracle.compress(plain[3], 1, oracle.dfZlib), oracle.compress(text, 1, oracle.dfGzip, fname_len=3),
             zlib.compress(plain[7], 9), oracle.compress(plain[5], -1, oracle.dfGzip, fname_len=0)]
    outs, sts = eng.uncompress_batch(mixed)
    assert sts == [0, 0, 0, 0] and outs == [plain[3], text, plain[7], plain[5]]


def check_plan_slots_with_gaps(eng, upload, download, alloc, levels=(1, -2, 0, 6), fills=(0xAB, 0xFF)):
    """Device plan API (include/zippy_hip.h): output slots at odd offsets in memory the caller has filled with a
    pattern -- nothing is cleared beforehand (round 6: the layout kernels zero exactly the words that are OR-ed into,
    csrc/zh_huffman.hip), so a stream's bytes must be the oracle's whatever was there, and NOTHING else may change:
    neither the rest of a slot nor the caller's bytes between slots.  Compressed, fixed, stored (two chunks) and
    empty buffers, the three containers; a misaligned d_dst is refused.  upload(bytes) -> (ptr, keep),
    alloc(n, fill) -> (ptr, keep), download(keep) -> bytes."""
    import pytest
    from zippy_amd.common import ZippyError
    rnd = np.random.default_rng(7).integers(0, 256, 70001, dtype=np.uint8).tobytes()
    srcs = [synth.corpus_file("alice29.txt")[:50000], b"", synth.corpus_file("html")[:33000], b"x" * 70001, rnd, b"ab",
            synth.corpus_file("alice29.txt")[:700]]
    src_off, pos = [], 0
    for s in srcs:
        src_off.append(pos)
        pos += len(s)
    d_src, keep_src = upload(b"".join(srcs) + b"\0" * 16)
    caps = [len(s) + len(s) // 8 + 2048 for s in srcs]
    dst_off, pos = [], 7
    for i, c in enumerate(caps):
        dst_off.append(pos)
        pos += c + (101, 1000, 3, 513, 0, 1, 2)[i]  # (slots 4 / 5: back to back at odd addresses)
    total = pos + 64
    plan = None
    for k, level in enumerate(levels):
        fmt = FORMATS[k % len(FORMATS)]
        fill = fills[k % len(fills)]
        d_dst, keep_dst = alloc(total, fill)
        plan = eng.plan_compress(src_off, [len(s) for s in srcs], dst_off, caps, level, fmt)
        plan.run(d_src, d_dst)
        lens, sts = plan.results()
        assert all(st == 0 for st in sts)
        got = download(keep_dst)
        mine = bytearray(total)
        for i, (s, o, ln) in enumerate(zip(srcs, dst_off, lens)):
            assert got[o:o + ln] == oracle.compress(s, level, fmt, fname_len=0), (level, fmt, i)
            mine[o:o + ln] = b"\1" * ln
        changed = [i for i in range(total) if not mine[i] and got[i] != fill]
        assert not changed, "level %d: bytes outside the streams changed, first at %d" % (level, changed[0])
    with pytest.raises(ZippyError):
        plan.run(d_src, d_dst + 1)


def check_plan_reruns(eng, upload, download, alloc, n, size):
    """A compress plan run three times (zh_l1_match.hip: from the second run on the BestSpeed matcher's waves take the
    cheapest fragments -- by what they cost the run before -- last; more fragments than waves here, so the order is a
    real one): every run's streams are the oracle's, byte for byte."""
    bufs = [b.tobytes() for b in synth.gen_batch("mix", n, size)]
    d_src, keep_src = upload(b"".join(bufs) + b"\0" * 16)
    cap = size + size // 8 + 2048
    slot = (cap + 255) & ~255
    d_dst, keep_dst = alloc(n * slot, 0)
    plan = eng.plan_compress([i * size for i in range(n)], [size] * n, [i * slot for i in range(n)], [cap] * n, 1, oracle.dfGzip)
    want = [oracle.compress(b, 1, oracle.dfGzip, fname_len=0) for b in bufs]
    for run in range(3):
        plan.run(d_src, d_dst)
        lens, sts = plan.results()
        assert all(st == 0 for st in sts), run
        got = download(keep_dst)
        for i, w in enumerate(want):
            assert lens[i] == len(w) and got[i * slot:i * slot + lens[i]] == w, (run, i)


def check_plan_pack(eng, upload, download, alloc):
    """zh_plan_pack / zh_plan_unpack (include/zippy_hip.h; zippy.nim:11-18: whole buffers are all that travels): a
    compress plan's results back to back with n + 1 device offsets == the oracle's streams concatenated (a failed
    buffer counts 0 bytes); the packed streams scattered into an uncompress plan's slots (another layout, odd offsets)
    decode to the inputs; a packed buffer that is too small is not overrun; a stream longer than its slot is cut to
    the slot and fails by itself."""
    import struct
    import pytest
    from zippy_amd.common import ZippyError
    srcs = [synth.corpus_file("alice29.txt")[:70000], b"", synth.corpus_file("html")[:33001], b"x" * 70001,
            synth.corpus_file("kppkn.gtb")[:150003], b"q"]
    n = len(srcs)
    src_off, pos = [], 0
    for s in srcs:
        src_off.append(pos)
        pos += len(s)
    d_src, keep_src = upload(b"".join(srcs) + b"\0" * 16)
    caps = [len(s) + len(s) // 8 + 2048 for s in srcs]
    caps[3] = 40  # too small: this buffer fails (ZH_ERR_DST_TOO_SMALL) and packs as 0 bytes
    dst_off, pos = [], 3
    for i, c in enumerate(caps):
        dst_off.append(pos)
        pos += c + (101, 1000, 3, 513, 77, 9)[i]
    d_dst, keep_dst = alloc(pos + 64, 0xAB)
    cplan = eng.plan_compress(src_off, [len(s) for s in srcs], dst_off, caps, 1, oracle.dfGzip)
    cplan.run(d_src, d_dst)
    want = [oracle.compress(s, 1, oracle.dfGzip, fname_len=0) for s in srcs]
    want[3] = b""
    total = sum(len(w) for w in want)
    d_pack, keep_pack = alloc(total + 64, 0xCD)
    d_offs, keep_offs = alloc(8 * (n + 1), 0xEE)
    cplan.pack(d_dst, d_pack, total + 64, d_offs)   # (no results() in between: the lengths are the device's)
    lens, sts = cplan.results()
    assert [st == 0 for st in sts] == [True, True, True, False, True, True]
    offs = list(struct.unpack("<%dQ" % (n + 1), download(keep_offs)))
    assert offs == [sum(len(w) for w in want[:i]) for i in range(n + 1)]
    packed = download(keep_pack)
    assert packed[:total] == b"".join(want)
    assert packed[total:] == b"\xcd" * 64, "bytes behind the packed streams changed"
    # too small a packed buffer: the offsets say so, nothing behind the capacity is written
    small = total - 1000
    d_pack2, keep_pack2 = alloc(total + 64, 0xCD)
    cplan.pack(d_dst, d_pack2, small, d_offs)
    cplan.results()
    assert struct.unpack("<%dQ" % (n + 1), download(keep_offs))[n] == total > small
    p2 = download(keep_pack2)
    assert p2[:small] == b"".join(want)[:small] and p2[small:] == b"\xcd" * (total + 64 - small)
    # ... and back: into an uncompress plan's source slots (sizes and places of their own), then decoded
    ucaps = [len(w) + (5, 0, 300, 64, 1, 17)[i] for i, w in enumerate(want)]
    ucaps[4] = len(want[4]) - 10  # a slot smaller than its stream: cut, and the stream fails alone
    usrc_off, pos = [], 5
    for c in ucaps:
        usrc_off.append(pos)
        pos += c + 13
    d_usrc, keep_usrc = alloc(pos + 64, 0x11)
    out_caps = [max(len(s), 1) for s in srcs]
    out_off, pos = [], 0
    for c in out_caps:
        out_off.append(pos)
        pos += c + 7
    d_out, keep_out = alloc(pos + 64, 0x22)
    uplan = eng.plan_uncompress(usrc_off, ucaps, out_off, out_caps, oracle.dfGzip)
    uplan.unpack(d_pack, d_offs, d_usrc)
    uplan.run(d_usrc, d_out)
    ulens, usts = uplan.results()
    got = download(keep_out)
    for i, s in enumerate(srcs):
        if i in (3, 4):  # the empty stream of the failed buffer; the cut stream
            assert usts[i] != 0
        else:
            assert usts[i] == 0 and got[out_off[i]:out_off[i] + ulens[i]] == s, i
    staged = download(keep_usrc)
    for i, w in enumerate(want):
        k = min(len(w), ucaps[i])
        assert staged[usrc_off[i]:usrc_off[i] + k] == w[:k]
        assert staged[usrc_off[i] + k:usrc_off[i] + k + 13] == b"\x11" * 13, "bytes outside a source slot changed"
    with pytest.raises(ZippyError):
        cplan.unpack(d_pack, d_offs, d_usrc)  # (a compress plan has no streams to be handed)


def split_inflate_edge_streams():
    """Streams that exercise the corners of the parallel token decode (csrc/zh_inflate_split.hip):
    periodic data (wrong starts never fall in step: the all-starts pass), hundreds of tiny blocks
    with empty stored blocks between them (Z_FULL_FLUSH), fixed-Huffman blocks, long distance codes,
    block ends near subchunk / superchunk borders, stored + compressed blocks mixed."""
    rnd = random.Random(77)
    out = []

    def z(data, level=6, wbits=31, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0):
        c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
        if not flush_every:
            return c.compress(data) + c.flush()
        parts = []
        for o in range(0, len(data), flush_every):
            parts.append(c.compress(data[o:o + flush_every]))
            parts.append(c.flush(zlib.Z_FULL_FLUSH if (o // flush_every) % 3 else zlib.Z_SYNC_FLUSH))
        parts.append(c.flush())
        return b"".join(parts)

    text = synth.corpus_file("alice29.txt")
    geo = synth.corpus_file("geo.protodata")
    for per in (1, 2, 3, 7, 8, 9, 31, 32, 33, 255, 256, 257, 258, 259, 1000):
        pat = rnd.randbytes(per)
        data = (pat * (300000 // per + 1))[:300000]
        out.append((z(data, rnd.choice((1, 6, 9))), data))
    out.append((z(b"\0" * 3000000, 6), b"\0" * 3000000))
    out.append((z(text, 6, flush_every=100), text))                  # ~1500 blocks
    out.append((z(geo, 9, flush_every=1777), geo))
    out.append((z(text[:70000], 6, strategy=zlib.Z_FIXED), text[:70000]))
    out.append((z(geo, 1, strategy=zlib.Z_HUFFMAN_ONLY), geo))
    out.append((z(text, 1, strategy=zlib.Z_RLE), text))
    big = text + rnd.randbytes(200000) + geo + bytes(100000) + text[::-1] + rnd.randbytes(70000)
    for lvl in (1, 6, 9):
        out.append((z(big, lvl), big))
    out.append((z(big, 6, wbits=15), big))
    out.append((z(big, 6, wbits=-15), big))
    # block ends walked across every bit position of a subchunk border: prefix lengths of one text
    for n in range(16370, 16400):
        out.append((z(text[:n], 6), text[:n]))
    return out


def damaged_header_streams(step=1):
    """Raw deflate streams (no checksum behind them: only the byte comparison catches a wrong byte) whose
    dynamic header is hit bit by bit: every bit of the first 90 bytes flipped, one at a time -- HLIT / HDIST /
    HCLEN, the code-length code's lengths, the run-length coded lengths with their repeat counts.  One input
    has a skewed alphabet (code lengths up to 15: second-level tables), one is text, one uses few symbols
    (long zero runs in the header).  zh_inflate_split.hip reads clean headers with a whole wave and builds the
    tables with the workgroup; anything else goes to the serial reader: both have to agree with the oracle."""
    rnd = random.Random(4242)
    skew = bytes(min(255, int(rnd.expovariate(0.035))) for _ in range(6000))
    few = bytes(rnd.choice(b"ab\x00\xff") for _ in range(2500)) + b"abab" * 50
    text = synth.corpus_file("alice29.txt")[:4000]
    out = []
    for data, strategy in ((skew, zlib.Z_HUFFMAN_ONLY), (text, zlib.Z_DEFAULT_STRATEGY), (few, zlib.Z_DEFAULT_STRATEGY)):
        c = zlib.compressobj(9, zlib.DEFLATED, -15, 9, strategy)
        blob = c.compress(data) + c.flush()
        assert (blob[0] >> 1) & 3 == 2, "expected a dynamic block"
        out.append(blob)
        for bit in range(0, min(len(blob), 90) * 8, step):
            m = bytearray(blob)
            m[bit >> 3] ^= 1 << (bit & 7)
            out.append(bytes(m))
    return out


def check_damaged_headers(eng, step=1):
    check_errors_match_oracle(eng, damaged_header_streams(step), oracle.dfDeflate)


def check_split_inflate_edges(eng):
    """Both inflate paths return the input for every stream above, and the same statuses when the
    output slot is one byte short (device plan API is exercised by check_plan_slots_with_gaps)."""
    cases = split_inflate_edge_streams()
    gz = [c for c in cases if c[0][:2] == b"\x1f\x8b"]
    outs, sts = eng.uncompress_batch([c[0] for c in gz], oracle.dfGzip)
    for (blob, want), got, st in zip(gz, outs, sts):
        assert st == 0 and got == want, (len(blob), len(want), st)
        assert oracle.uncompress(blob, oracle.dfGzip) == want
    zl = [c for c in cases if c[0][:2] != b"\x1f\x8b"]
    for blob, want in zl:
        fmt = oracle.dfZlib if (blob[0] & 0x0f) == 8 and (blob[0] * 256 + blob[1]) % 31 == 0 else oracle.dfDeflate
        got, st = eng.uncompress_batch([blob], fmt)
        assert st == [0] and got[0] == want, (len(blob), fmt, st)


def stored_chain_streams(nblocks=70, small=False):
    """Streams of stored blocks (inflate.nim:252-266), the kind incompressible data makes -- one of 65 535 bytes after
    the other (deflate.nim:186-199) --, for the chain reader of the tokens kernel (64 headers at once) and the
    writer's grouped copy: whole chains of more than 64 blocks, a short last block, an empty one, chains broken by a
    compressed block, by a short block in the middle, and damaged ones (a length that does not match its complement
    in the middle of a chain, a chain that runs past the input).  small: the subset the CPU emulator (a third of a
    megabyte a second on these) runs; the GPU tests run all of them.  -> [(raw deflate, plain or None)]"""
    rnd = random.Random(4711)
    noise = rnd.randbytes(nblocks * 65535 + 12345)

    def stored(data, final, size=65535):
        out = []
        chunks = [data[o:o + size] for o in range(0, len(data), size)] or [b""]
        for k, c in enumerate(chunks):
            out.append(bytes([1 if final and k == len(chunks) - 1 else 0]) + struct.pack("<HH", len(c), len(c) ^ 0xffff) + c)
        return b"".join(out)
    text = synth.corpus_file("alice29.txt")[:50000]
    dyn = zlib.compressobj(6, zlib.DEFLATED, -15)
    dyn_block = dyn.compress(text) + dyn.flush(zlib.Z_FULL_FLUSH)  # (ends byte-aligned with an empty stored block, not final)
    out = []
    out.append((stored(noise, True), noise))                                        # the oracle's own shape at level 0
    if not small:
        out.append((oracle.compress(noise, 0, oracle.dfDeflate), noise))
    out.append((oracle.compress(noise[:200000], 1, oracle.dfDeflate), noise[:200000]))  # incompressible at level 1: stored
    if not small:
        out.append((stored(noise[:65535 * 64], True), noise[:65535 * 64]))          # exactly 64 full blocks, the last final
    out.append((stored(noise[:65535 * 65], False) + stored(b"", True), noise[:65535 * 65]))  # an empty final block behind the chain
    out.append((stored(noise[:65535 * 3], False) + dyn_block + stored(noise[:65535 * (nblocks - 1) + 5], True),
                noise[:65535 * 3] + text + noise[:65535 * (nblocks - 1) + 5]))
    if not small:
        out.append((stored(noise[:65535 * 5], False) + stored(noise[:1000], False, 1000) + stored(noise[:65535 * 65], True),
                    noise[:65535 * 5] + noise[:1000] + noise[:65535 * 65]))
    out.append((stored(noise[:300000], True, 30000), noise[:300000]))               # no full block at all
    good = stored(noise[:65535 * (20 if small else 40)], True)
    bad = bytearray(good)
    bad[17 * 65540 + 3] ^= 0x40                                                     # block 17: NLEN no longer the complement
    out.append((bytes(bad), None))
    out.append((good[:-30000], None))                                               # the last block runs past the input
    bad = bytearray(good)
    bad[9 * 65540] |= 0x06                                                          # block 9: BTYPE 3
    out.append((bytes(bad), None))
    return out


def check_stored_chains(eng, nblocks=70, small=False):
    """The streams above through the device decoder: bytes where they are sound (and through zlib, the referee), the
    oracle's accept / reject decision where they are not; and with an output slot that is too small the status a
    caller grows its buffer on, not another."""
    cases = stored_chain_streams(nblocks, small)
    outs, sts = eng.uncompress_batch([c[0] for c in cases], oracle.dfDeflate)
    for (blob, want), got, st in zip(cases, outs, sts):
        try:
            ref = oracle.uncompress(blob, oracle.dfDeflate)
        except oracle.ZippyError:
            ref = None
        assert ref == want, "the oracle disagrees with the test's expectation"
        assert (st == 0) == (want is not None), (len(blob), st)
        if want is not None:
            assert got == want and zlib.decompress(blob, -15) == want
    one = [cases[1 if small else 0][0]]  # (a batch of one: the wide kernels)
    got, st = eng.uncompress_batch(one, oracle.dfDeflate)
    assert st == [0] and got[0] == cases[1 if small else 0][1]


def check_stored_chain_segmented(eng, monkeypatch, nblocks=70, text_bytes=600000):
    """A chain of full stored blocks in the MIDDLE of a stream that is decoded segment-wise (zh_inflate_seg.hip): the
    segments inside the chain have no block start, the decoder before them reads the chain 64 headers a step and has to
    stop where the next segment's found start is -- the compressed blocks behind the chain."""
    monkeypatch.setenv("ZH_SEG_MIN", "65536")
    monkeypatch.setenv("ZH_SEG_BYTES", "16384")
    monkeypatch.setenv("ZH_SEG_SETUP", "0")
    rnd = random.Random(99)
    noise = rnd.randbytes(nblocks * 65535)
    text = synth.gen_batch("text", 1, text_bytes, first_index=3)[0].tobytes()

    def dyn(data, last):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        return c.compress(data) + (c.flush() if last else c.flush(zlib.Z_FULL_FLUSH))
    stored = b"".join(bytes([0]) + struct.pack("<HH", 65535, 0) + noise[o:o + 65535] for o in range(0, len(noise), 65535))
    last = bytes([1]) + struct.pack("<HH", 777, 777 ^ 0xffff) + noise[:777]
    for blob, want, holds in ((dyn(text, False) + stored + dyn(text[::-1], True), text + noise + text[::-1], None),
                              (stored + dyn(text, True), noise + text, None),
                              # nothing but stored blocks (incompressible data): chained stored blocks are segment
                              # starts too, so this stream IS decoded by many workgroups
                              (stored + last, noise + noise[:777], True)):
        assert zlib.decompress(blob, -15) == want
        before = eng.segment_stats()
        outs, sts = eng.uncompress_batch([blob], oracle.dfDeflate)
        assert sts == [0] and outs[0] == want
        cut, held = eng.segment_stats()
        assert cut - before[0] == 1, "the stream was not cut into segments"
        if holds:
            assert held - before[1] == 1, "a chain of stored blocks left to one workgroup"
    for k in ("ZH_SEG_MIN", "ZH_SEG_BYTES", "ZH_SEG_SETUP"):
        monkeypatch.delenv(k)


def segmented_streams(scale):
    """Foreign streams for the segment-wise decoder (zh_inflate_seg.hip): many blocks each, the
    kinds of block boundaries it has to cope with.  -> [(blob, format, plain)]"""
    rng = random.Random(77)
    text = synth.gen_batch("text", 1, 96 * scale, first_index=5)[0].tobytes()
    mix = synth.gen_batch("mix", 1, 64 * scale, first_index=6)[0].tobytes()
    runs = synth.gen_batch("runs", 1, 192 * scale, first_index=7)[0].tobytes()
    noise = bytes(rng.getrandbits(8) for _ in range(8 * scale))

    def blocks(plain, level, wbits, flushes, every, strategy=zlib.Z_DEFAULT_STRATEGY):
        c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
        parts = []
        for k, o in enumerate(range(0, len(plain), every)):
            parts.append(c.compress(plain[o:o + every]))
            parts.append(c.flush(flushes[k % len(flushes)]))
        parts.append(c.flush())
        return b"".join(parts)

    out = [(zlib.compress(text, 6), oracle.dfZlib, text)]  # two blocks: one decoder does it all
    # blocks that end anywhere in a byte (Z_BLOCK) and copies that reach back across them
    out.append((blocks(text + mix, 6, -15, [zlib.Z_BLOCK], 2500), oracle.dfDeflate, text + mix))
    out.append((blocks(mix + text, 1, 15, [zlib.Z_BLOCK, zlib.Z_SYNC_FLUSH, zlib.Z_BLOCK, zlib.Z_FULL_FLUSH], 3000),
                oracle.dfZlib, mix + text))
    # fixed-code blocks only: no block start is ever found
    out.append((blocks(mix, 6, -15, [zlib.Z_BLOCK], 3000, zlib.Z_FIXED), oracle.dfDeflate, mix))
    # stored blocks (incompressible stretches) between compressed ones; a zlib stream inside, whose
    # block headers sit byte-aligned in stored blocks of the outer stream
    inner = blocks(text[: 24 * scale], 6, 15, [zlib.Z_BLOCK], 2000)
    plain = text[: 20 * scale] + noise + inner + mix[: 20 * scale] + noise + inner + text[20 * scale: 40 * scale]
    out.append((blocks(plain, 6, 31, [zlib.Z_BLOCK], 4000), oracle.dfGzip, plain))
    # long runs: a few bits per token, back-to-back maximal matches
    plain = b"\0" * (64 * scale) + text[: 8 * scale] + b"ab" * (32 * scale) + runs
    out.append((blocks(plain, 6, 15, [zlib.Z_BLOCK], 20000), oracle.dfZlib, plain))
    return out


def check_segmented(eng, scale, monkeypatch, seg_bytes):
    """Large streams on many workgroups: same bytes and statuses as the one-workgroup decode, for
    whole streams, streams cut short and streams with a flipped bit."""
    monkeypatch.setenv("ZH_SEG_MIN", str(4 * seg_bytes))
    monkeypatch.setenv("ZH_SEG_BYTES", str(seg_bytes))
    monkeypatch.setenv("ZH_SEG_SETUP", "0")  # (the set-up cost that keeps small jobs off this path)
    cases = segmented_streams(scale)
    n_foreign = len(cases)
    # this library's own streams: ONE block (the last one) however long -- every decoder but the
    # first starts inside it; raw deflate has no checksum to catch a wrong byte, only this comparison
    own_src = [synth.gen_batch(kind, 1, 72 * scale, first_index=9)[0].tobytes() for kind in ("text", "mix")]
    for fmt in (oracle.dfDeflate, oracle.dfZlib, oracle.dfGzip):
        for level in (1, 6):
            comp, sts = eng.compress_batch(own_src, level, fmt)
            assert sts == [0, 0]
            cases += [(c, fmt, p) for c, p in zip(comp, own_src) if len(c) >= 4 * seg_bytes]
    n_own = len(cases) - n_foreign
    held_foreign = 0
    for i, (blob, fmt, plain) in enumerate(cases):
        assert len(blob) >= 4 * seg_bytes, len(blob)
        before = eng.segment_stats()
        outs, sts = eng.uncompress_batch([blob], fmt)
        assert sts == [0] and outs[0] == plain, (fmt, len(blob), sts)
        # ... and by MANY workgroups: a chain of segments that does not hold is decoded by one workgroup, with the same
        # bytes -- only the count tells (zh_debug_segment_stats).  This library's own streams always hold; a foreign
        # one with fewer than four block starts (fixed codes, one block) legitimately does not.
        cut, held = (a - b for a, b in zip(eng.segment_stats(), before))
        assert cut >= 1, (i, cut)
        if i >= n_foreign:
            assert held == cut, ("own stream left to one workgroup", i, fmt, len(blob), cut, held)
        else:
            held_foreign += held == cut
    assert held_foreign >= n_foreign - 1, (held_foreign, n_foreign)
    # Bits of the payload that read like a block header and are none (about one a GiB; ZH_SEG_FAKE_START plants one):
    # the decoder before runs past it, the segments behind it still find their sub-starts (from the real header, one
    # found start further back), and the stream is still decoded segment-wise -- such a guess once cost a 1 GiB
    # stream of this library a factor of 100 (tools/gpu_big_buffer.py).
    for blob, fmt, plain in cases[n_foreign:n_foreign + 2]:
        for fake_bit in (len(blob) * 2 + 3, len(blob) * 9 // 2):
            monkeypatch.setenv("ZH_SEG_FAKE_START", str(fake_bit))
            before = eng.segment_stats()
            outs, sts = eng.uncompress_batch([blob], fmt)
            cut, held = (a - b for a, b in zip(eng.segment_stats(), before))
            assert sts == [0] and outs[0] == plain and cut >= 1 and held == cut, (fmt, len(blob), fake_bit, sts, cut, held)
    # ... and such a guess just BEFORE a real block start of the same segment (blocks of many segments: the block-parallel
    # form's, 32 KiB of input each): a segment reports the lowest position that passes for a start, so the guess used to
    # hide the start every segment of the block behind it needs; a segment keeps two candidates now and the first is
    # probed (a superchunk decoded) before anybody relies on it
    if seg_bytes <= 2048:
        src = synth.gen_batch("text", 1, 200 * scale, first_index=3)[0].tobytes()
        blob, index = eng.compress_blocks(src, 1, oracle.dfGzip, 32 * scale)
        for j in (2, 4):
            for back in (40, 300):
                monkeypatch.setenv("ZH_SEG_FAKE_START", str(index[j][0] - back))
                before = eng.segment_stats()
                outs, sts = eng.uncompress_batch([blob], oracle.dfGzip)
                cut, held = (a - b for a, b in zip(eng.segment_stats(), before))
                assert sts == [0] and outs[0] == src and cut >= 1 and held == cut, (j, back, sts, cut, held)
    monkeypatch.delenv("ZH_SEG_FAKE_START")
    # a batch of them at once (same format), small streams (no segments) in between: zlib streams
    zl = [c for c in cases if c[1] == oracle.dfZlib]
    small = [(zlib.compress(c[2][:k], 6), c[1], c[2][:k]) for c, k in zip(zl, (0, 1, 3000))]
    mixed = [x for pair in zip(zl, small) for x in pair]
    outs, sts = eng.uncompress_batch([c[0] for c in mixed], oracle.dfZlib)
    assert sts == [0] * len(mixed) and all(o == c[2] for o, c in zip(outs, mixed))
    # damage: the statuses are those of the ordinary decoder
    rng = random.Random(3)
    blob, fmt, plain = cases[1]
    bad = [blob[: len(blob) * 2 // 3], blob[:-5]]
    for _ in range(10):
        b = bytearray(blob)
        b[rng.randrange(8, len(b) - 8)] ^= 1 << rng.randrange(8)
        bad.append(bytes(b))
    monkeypatch.setenv("ZH_SEG", "0")
    want = [eng.uncompress_batch([b], fmt) for b in bad]
    monkeypatch.setenv("ZH_SEG", "1")
    got = [eng.uncompress_batch([b], fmt) for b in bad]
    for b, w, g_ in zip(bad, want, got):
        assert w[1] == g_[1], (len(b), w[1], g_[1])
        if w[1] == [0]:
            assert w[0] == g_[0]


# ---- the checksum kernels (csrc/zh_checksum.hip) against zlib.crc32 / zlib.adler32, which are exact: every length,
# alignment and piece count at which the kernels take another path.  The borders below are the row sizes of the three
# lane widths the kernel can be built with (1024 / 2048 / 4096), their neighbours, and the 32 KiB piece: written out,
# not derived from the kernel's constants. ----
CK_BORDERS = (512, 1024, 2048, 4096, 6144, 30720, 32768, 34816, 65536)
ZH_ERR_CHECKSUM, ZH_ERR_DST_TOO_SMALL = 8, 21


def checksum_lengths():
    """L: 0..130, every border -17..+17, three pieces plus a byte"""
    out = set(range(131))
    for b in CK_BORDERS:
        out.update(range(b - 17, b + 18))
    out.add(98305)
    return sorted(out)


def checksum_lengths_aligned(small=False):
    """L_a: 0..48, B-1, B, B+1, B+15, B+16, B+17 of every border, 98305.  small: the lengths up to 6200 and 32768,
    32769, 65537."""
    out = set(range(49))
    for b in CK_BORDERS:
        out.update((b - 1, b, b + 1, b + 15, b + 16, b + 17))
    out.add(98305)
    if small:
        out = {n for n in out if n <= 6200 or n in (32768, 32769, 65537)}
    return sorted(out)


_ck_pools = {}


def checksum_fill(kind, n):
    """n bytes of a fill: 'rand' (seeded), 'ff' (the largest Adler sums), 'zero' (a CRC that depends on the length
    alone: the conditioning terms), 'text' (corpus text for the matcher)"""
    if kind not in _ck_pools:
        if kind == "rand":
            _ck_pools[kind] = np.random.default_rng(20260).integers(0, 256, 12 << 20, dtype=np.uint8).tobytes()
        elif kind == "text":
            _ck_pools[kind] = synth.corpus_file("alice29.txt")
        else:
            _ck_pools[kind] = {"ff": b"\xff", "zero": b"\x00"}[kind] * (12 << 20)
    pool = _ck_pools[kind]
    assert n <= len(pool)
    return pool[:n]


def check_checksum_lengths(eng, small=False):
    """Host path (zh_crc32_batch, zh_adler32; every buffer at a 256-byte aligned address: head 0): every length of L,
    one zh_crc32_batch call a fill with empty buffers first, last and in between; zh_adler32 a call a length.
    small: the random fill only."""
    lens = checksum_lengths()
    for kind in ("rand",) if small else ("rand", "ff", "zero"):
        bufs = [b""]
        for k, n in enumerate(lens):
            bufs.append(checksum_fill(kind, n))
            if k % 40 == 7:
                bufs.append(b"")
        bufs.append(b"")
        got = eng.crc32_batch(bufs)
        bad = [(len(b), hex(g)) for b, g in zip(bufs, got) if g != zlib.crc32(b)]
        assert not bad, ("crc32_batch", kind, bad[:8])
    for kind in ("rand",) if small else ("rand", "ff"):
        bad = []
        for n in lens:
            b = checksum_fill(kind, n)
            g = eng.adler32(b)
            if g != zlib.adler32(b):
                bad.append((n, hex(g)))
        assert not bad, ("adler32", kind, bad[:8])


def _ck_pack_sources(srcs, aligns, pad=0xA7):
    """One blob with srcs[i] at an offset that is aligns[i] (mod 16), 16 spare bytes in front and 64 behind (the plans
    read whole words around a source) -> (blob, offsets)"""
    blob = bytearray(bytes([pad]) * 16)
    offs = []
    for s, a in zip(srcs, aligns):
        blob += bytes([pad]) * ((a - len(blob)) % 16)
        offs.append(len(blob))
        blob += s
    blob += bytes([pad]) * 64
    return bytes(blob), offs


def _ck_compress_plan(eng, d_src, soff, srcs, level, fmt, alloc, download, want_crcs=True):
    """One compress plan over srcs -> (streams, statuses, crcs)"""
    caps = [eng.compress_bound(len(s), fmt) for s in srcs]
    doff, pos = [], 4
    for c in caps:
        doff.append(pos)
        pos += c + 5
    d_dst, keep = alloc(pos + 64, 0x5A)
    plan = eng.plan_compress(soff, [len(s) for s in srcs], doff, caps, level, fmt)
    if want_crcs:
        plan.request_crc32()
    plan.run(d_src, d_dst)
    lens, sts = plan.results()
    crcs = plan.crc32() if want_crcs else None
    got = download(keep)
    plan.close()
    return [got[o:o + n] for o, n in zip(doff, lens)], sts, crcs


def check_checksum_alignment(eng, upload, download, alloc, small=False):
    """Compress plans whose sources start at every address mod 16 (the kernel's head of 0..15 bytes, taken by one lane;
    the host calls only ever give it head 0): level 0, one dfGzip and one dfZlib plan over every length of L_a at every
    alignment -- trailer CRC-32 / ISIZE / Adler-32 against zlib, zh_plan_crc32 of both plans (the zlib plan then makes
    both checksums in one launch), the whole stream against the oracle; then alignments 0, 5, 15 at level 1 on text,
    the checksum beside the matcher.  small: alignments 0, 1, 15 and checksum_lengths_aligned(small=True)."""
    eng.set_gzip_fname_len(0)
    lens = checksum_lengths_aligned(small)
    for kind, level, aligns in (("rand", 0, (0, 1, 15) if small else range(16)), ("ff", 0, (0, 1, 15) if small else range(16)),
                                ("text", 1, (0, 5, 15))):
        srcs = [checksum_fill(kind, n) for a in aligns for n in lens]
        want_a = [a for a in aligns for n in lens]
        blob, soff = _ck_pack_sources(srcs, want_a)
        d_src, keep_src = upload(blob)
        assert [(d_src + o) % 16 for o in soff] == want_a, "a source is not at the address (mod 16) it is meant to test"
        for fmt in (oracle.dfGzip, oracle.dfZlib) if level == 0 else (oracle.dfGzip,):
            outs, sts, crcs = _ck_compress_plan(eng, d_src, soff, srcs, level, fmt, alloc, download)
            for i, (s, out) in enumerate(zip(srcs, outs)):
                at = (kind, level, fmt, "align", want_a[i], "len", len(s))
                assert sts[i] == 0, at + (sts[i],)
                if fmt == oracle.dfGzip:
                    assert struct.unpack("<II", out[-8:]) == (zlib.crc32(s), len(s)), at + ("gzip trailer",)
                else:
                    assert struct.unpack(">I", out[-4:])[0] == zlib.adler32(s), at + ("zlib trailer",)
                assert crcs[i] == zlib.crc32(s), at + ("zh_plan_crc32",)
                assert out == oracle.compress(s, level, fmt, fname_len=0), at + ("stream",)
                if level != 0:
                    assert zlib.decompress(out, WBITS[fmt]) == s, at


def _ck_streams(data, wbits):
    c = zlib.compressobj(1, zlib.DEFLATED, wbits)
    return c.compress(data) + c.flush()


def check_checksum_uncompress(eng, upload, download, alloc, small=False):
    """Uncompress plans: the piece length comes from the device (dyn_len) and is clamped to the piece's share of the
    slot, and the verify step compares with the stored checksum.  zlib-made gzip and zlib streams of every length of
    L_a, each OUTPUT at every address mod 16, capacities of len + 0 / 1 / 40000 (clamped, empty and short last pieces),
    in memory filled with a pattern; a dfGzip, a dfZlib and a dfDetect plan (both kinds interleaved), zh_plan_crc32 on
    each.  Then: a bit of the stored checksum flipped in every third stream (status 8, the oracle rejects them too);
    every fifth slot one byte short (status 21; neighbours and guard bytes untouched); the statuses from
    zh_plan_device_statuses; and the first run as two halves (ZH_INFLATE_HALVES: the first half's checksum launch).
    small: alignments 0, 1, 15, checksum_lengths_aligned(small=True), one fill a stream in turn (the full case runs
    the random and the 0xFF fill whole)."""
    import ctypes
    PAT = 0xC3
    lens = checksum_lengths_aligned(small)
    aligns = (0, 1, 15) if small else range(16)
    want_a = [a for a in aligns for n in lens]
    n = len(want_a)
    for kinds in (("rand", "ff", "zero"),) if small else (("rand",), ("ff",)):
        datas = [checksum_fill(kinds[i % len(kinds)], ln) for i, ln in enumerate(lens * len(aligns))]
        per_kind = {wb: [_ck_streams(d, wb) for d in datas] for wb in (31, 15)}
        for d, g, z in zip(datas[::7], per_kind[31][::7], per_kind[15][::7]):  # (the premise: what zlib made, zlib reads)
            assert zlib.decompress(g, 31) == d and zlib.decompress(z, 15) == d

        def flipped(blob, wb, i):
            b = bytearray(blob)
            b[len(b) - (8 if wb == 31 else 4) + i % 4] ^= 1 << (i % 8)  # the CRC-32 / Adler-32 field, not ISIZE
            return bytes(b)
        bad_kind = {wb: [flipped(b, wb, i) if i % 3 == 0 else b for i, b in enumerate(per_kind[wb])] for wb in (31, 15)}
        for wb, fmt in ((31, oracle.dfGzip), (15, oracle.dfZlib)):
            for i in range(0, n, 3):
                try:
                    oracle.uncompress(bad_kind[wb][i], fmt)
                    assert False, ("the oracle accepts a stream with a flipped checksum", wb, len(datas[i]))
                except oracle.ZippyError:
                    pass
        # sources: gzip streams, zlib streams, and both with the flipped ones, in one blob
        groups = [per_kind[31], per_kind[15], bad_kind[31], bad_kind[15]]
        flat = [b for g in groups for b in g]
        blob, soff = _ck_pack_sources(flat, [(5 * i) % 16 for i in range(len(flat))])
        d_src, keep_src = upload(blob)
        goff = [soff[k * n:(k + 1) * n] for k in range(4)]

        def layout(caps):  # (for memory that starts at a multiple of 16: checked against the pointer below)
            off, pos = [], 16
            for a, c in zip(want_a, caps):
                pos += (a - pos) % 16
                off.append(pos)
                pos += c + 3
            return off, pos + 64

        def run(plan_fmt, pick, caps, bad_every=0):
            """pick(i) -> index of the source group of stream i; -> (lens, sts, crcs, device statuses, output memory, offsets)"""
            off, total = layout(caps)
            d_dst, keep = alloc(total, PAT)
            assert [(d_dst + o) % 16 for o in off] == want_a, "an output is not at the address (mod 16) it is meant to test"
            plan = eng.plan_uncompress([goff[pick(i)][i] for i in range(n)], [len(groups[pick(i)][i]) for i in range(n)],
                                       off, caps, plan_fmt)
            plan.request_crc32()
            plan.run(d_src, d_dst)
            olens, sts = plan.results()
            crcs = plan.crc32()
            host = (ctypes.c_int32 * n)()
            eng._check(eng.lib.zh_device_download(eng._h, host, plan.device_statuses(), n * 4))
            got = np.frombuffer(download(keep), np.uint8)
            plan.close()
            return olens, sts, crcs, list(host), got, off

        def expect(plan_name, res, caps, failing, status):
            """streams in `failing` end with `status`, all others with 0, their bytes and CRC-32; nothing outside the
            slots of the failing ones and the outputs of the others differs from the pattern"""
            olens, sts, crcs, dev_sts, got, off = res
            assert dev_sts == sts, (plan_name, "zh_plan_device_statuses differs from zh_plan_results")
            want = np.full(len(got), PAT, np.uint8)
            care = np.ones(len(got), bool)
            for i, d in enumerate(datas):
                at = (plan_name, kinds[i % len(kinds)], "align", want_a[i], "len", len(d), "cap", caps[i])
                if i in failing:
                    assert sts[i] == status, at + (sts[i],)
                    care[off[i]:off[i] + caps[i]] = False  # (the slot of a failed stream is its own to scribble in)
                    continue
                assert sts[i] == 0, at + (sts[i],)
                assert olens[i] == len(d), at + (olens[i],)
                assert crcs[i] == zlib.crc32(d), at + ("zh_plan_crc32", hex(crcs[i]))
                want[off[i]:off[i] + len(d)] = np.frombuffer(d, np.uint8)
            diff = np.nonzero((got != want) & care)[0]
            if len(diff):
                k = max(i for i in range(n) if off[i] <= diff[0]) if diff[0] >= off[0] else -1
                assert False, (plan_name, "memory differs at", int(diff[0]), "stream", k, "at", off[k], "len", len(datas[k]))

        plans = (("gzip", oracle.dfGzip, lambda i: 0), ("zlib", oracle.dfZlib, lambda i: 1),
                 ("detect", oracle.dfDetect, lambda i: i % 2))
        caps = [len(d) + (0, 1, 40000)[i % 3] for i, d in enumerate(datas)]
        short = {i for i, d in enumerate(datas) if i % 5 == 0 and len(d) >= 1}
        caps_short = [len(d) - 1 if i in short else c for i, (d, c) in enumerate(zip(datas, caps))]
        for name, fmt, pick in plans:
            expect(name, run(fmt, pick, caps), caps, (), 0)
            expect(name + ", flipped checksums", run(fmt, lambda i: pick(i) + 2, caps), caps, set(range(0, n, 3)), ZH_ERR_CHECKSUM)
            expect(name + ", slots one byte short", run(fmt, pick, caps_short), caps_short, short, ZH_ERR_DST_TOO_SMALL)
        old = os.environ.get("ZH_INFLATE_HALVES")
        os.environ["ZH_INFLATE_HALVES"] = "4"  # (read when a plan is made)
        try:
            for name, fmt, pick in plans:
                expect(name + ", two halves", run(fmt, pick, caps), caps, (), 0)
        finally:
            if old is None:
                del os.environ["ZH_INFLATE_HALVES"]
            else:
                os.environ["ZH_INFLATE_HALVES"] = old


CK_PIECE_COUNTS = (1, 2, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 256, 257, 258, 319, 320, 321)


def checksum_piece_count_sizes(small=False):
    """(np - 1) * 32768 + last bytes: last in turn 1, 32767, 32768, all three for np = 65, 129, 257, 321 (shares of 1
    to 6 pieces a lane, the table in LDS from 257 pieces on, lanes with a partial share, an empty one, and right-hand
    sides of exactly whole pieces).  small: np up to 258."""
    sizes, turn = [], 0
    for npieces in CK_PIECE_COUNTS:
        if small and npieces > 258:
            break
        if npieces in (65, 129, 257, 321):
            lasts = (1, 32767, 32768)
        else:
            lasts = ((1, 32767, 32768)[turn % 3],)
            turn += 1
        sizes += [(npieces - 1) * 32768 + last for last in lasts]
    return sizes


def check_checksum_piece_counts(eng, upload, download, alloc, small=False):
    """The combine kernel: buffers of checksum_piece_count_sizes() -- CRC-32 of all of them in ONE zh_crc32_batch call
    (first_piece indexing across buffers), Adler-32 a buffer a call (random bytes; 0xFF for the four largest); then
    65 and 257 pieces through a level 0 gzip plan with the source at an address of 7 (mod 16): a head and a ragged
    share in one run.  small: np up to 258, and 65 pieces alone through the plan."""
    sizes = checksum_piece_count_sizes(small)
    bufs = [checksum_fill("rand", n) for n in sizes]
    want = [zlib.crc32(b) for b in bufs]
    got = eng.crc32_batch(bufs)
    bad = [(n, -(-n // 32768), hex(g)) for n, g, w in zip(sizes, got, want) if g != w]
    assert not bad, ("crc32_batch: (bytes, pieces, got)", bad)
    bad = []
    for kind, some in (("rand", sizes), ("ff", sorted(sizes)[-4:])):
        for n in some:
            b = checksum_fill(kind, n)
            g = eng.adler32(b)
            if g != zlib.adler32(b):
                bad.append((kind, n, -(-n // 32768), hex(g)))
    assert not bad, ("adler32: (fill, bytes, pieces, got)", bad)
    eng.set_gzip_fname_len(0)
    srcs = [checksum_fill("rand", 64 * 32768 + 1)] + ([] if small else [checksum_fill("rand", 256 * 32768 + 32767)])
    blob, soff = _ck_pack_sources(srcs, [7] * len(srcs))
    d_src, keep_src = upload(blob)
    assert [(d_src + o) % 16 for o in soff] == [7] * len(srcs)
    outs, sts, crcs = _ck_compress_plan(eng, d_src, soff, srcs, 0, oracle.dfGzip, alloc, download)
    for s, out, st, crc in zip(srcs, outs, sts, crcs):
        assert st == 0
        assert struct.unpack("<II", out[-8:]) == (zlib.crc32(s), len(s) & 0xffffffff), ("gzip trailer", len(s))
        assert crc == zlib.crc32(s), ("zh_plan_crc32", len(s))
        assert zlib.decompress(out, 31) == s


def check_checksum_entry_points(eng, small=False):
    """zh_compress_batch_crc32 (dfDeflate, levels 1 and 0): the CRC-32s are zlib's, streams and statuses those of
    zh_compress_batch -- as one plan and as pipelined groups.  zh_uncompress_batch_sized with CRCs over the same inputs
    as raw deflate and zlib streams (Python's zlib), the hints in turn exact, 0, half the size (the retry pass, which
    fetches the CRCs of the streams it decodes again separately) and four times the size: outputs and statuses are
    zh_uncompress_batch's, the CRC-32s zlib's; a truncated stream in the middle fails alone.  small: inputs of at
    most 40 KB."""
    inputs = checksum_entry_point_inputs(small)
    want_crc = [zlib.crc32(b) for b in inputs]
    for pipe in ((1 << 60, 0), (1, 150000)):
        try:
            eng.set_host_pipeline(*pipe)
            for level in (1, 0):
                outs, sts, crcs = eng.compress_batch_crc32(inputs, level, oracle.dfDeflate)
                assert crcs == want_crc, (pipe, level, [len(b) for b, c, w in zip(inputs, crcs, want_crc) if c != w])
                assert (outs, sts) == eng.compress_batch(inputs, level, oracle.dfDeflate), (pipe, level)
                assert all(s == 0 for s in sts)
                for b, out in zip(inputs[::5], outs[::5]):
                    assert zlib.decompress(out, -15) == b
            for fmt, wb in ((oracle.dfDeflate, -15), (oracle.dfZlib, 15)):
                blobs = []
                for k, b in enumerate(inputs):
                    c = zlib.compressobj((1, 6, 9)[k % 3], zlib.DEFLATED, wb)
                    blobs.append(c.compress(b) + c.flush())
                cut = len(blobs) // 2
                blobs[cut] = blobs[cut][:len(blobs[cut]) * 2 // 3]  # truncated
                hints = [(len(b), 0, len(b) // 2, 4 * len(b))[k % 4] for k, b in enumerate(inputs)]
                outs, sts, crcs = eng.uncompress_batch_sized(blobs, fmt, hints)
                assert (outs, sts) == eng.uncompress_batch(blobs, fmt), (pipe, fmt)
                for k, b in enumerate(inputs):
                    if k == cut:
                        assert sts[k] != 0 and outs[k] is None, (pipe, fmt, sts[k])
                    else:
                        assert sts[k] == 0 and outs[k] == b, (pipe, fmt, k, len(b), sts[k])
                        assert crcs[k] == want_crc[k], (pipe, fmt, k, len(b), hints[k], hex(crcs[k]))
                outs2, sts2, none = eng.uncompress_batch_sized(blobs, fmt, hints, want_crcs=False)
                assert (outs2, sts2, none) == (outs, sts, None)
        finally:
            eng.set_host_pipeline(0, 0)


def checksum_entry_point_inputs(small=False):
    """edge_inputs() and three corpus slices of 70-200 KB (small: everything of at most 40 KB, the slices cut to it)"""
    inputs = edge_inputs() + [synth.corpus_file("alice29.txt")[:70001], synth.corpus_file("html")[1000:101000],
                              synth.corpus_file("kppkn.gtb")[:180000]]
    if small:
        inputs = [b for b in inputs[:-3] if len(b) <= 40000] + [b[:40000 - 777 * k] for k, b in enumerate(inputs[-3:])]
    return inputs


# ---- hand-built deflate streams (tests/deflate_craft.py): what no encoder emits.  Every case is
# (name, raw deflate, plain or None, status or None); the name's part before the "/" is its family. ----
def _t1_code():
    """Codes that reach 15 bits in both alphabets, both complete: literals 0..253 and the end of block at 8 bits,
    254 at 9, 255 at 10, lengths 257 / 258 / 259 at 11 / 12 / 13, 281..284 (five extra bits) at 15; distances
    0..13 at 1..14 bits, 28 and 29 (thirteen extra bits) at 15.  281..284 with 28 / 29 is a 48-bit token."""
    lit = [0] * 286
    for i in range(254):
        lit[i] = 8
    lit[254], lit[255], lit[256], lit[257], lit[258], lit[259] = 9, 10, 8, 11, 12, 13
    for i in range(281, 285):
        lit[i] = 15
    dist = [0] * 30
    for k in range(14):
        dist[k] = k + 1
    dist[28] = dist[29] = 15
    assert dc.kraft(lit) == 32768 and dc.kraft(dist) == 32768
    return lit, dist


def _craft_t1(s, ntokens, final, rnd):
    """A stored preamble of 32 KiB, then one dynamic block of ntokens tokens: runs of 32 back-to-back 48-bit tokens
    with a 9-bit literal between the runs (48 * 32 = 3 * 512 and 9 is a unit mod 16: 16 runs start a 48-bit token at
    every residue mod 512), then pairs and single ones between literals of 8, 9 and 10 bits."""
    s.stored(rnd.randbytes(32768), False)
    lit, dist = _t1_code()
    s.dynamic_block(lit, dist, final)
    n = [0]

    def tok():
        j = n[0]
        n[0] += 1
        sym = 281 + j % 4
        extra = 31 if j % 8 == 3 else (j * 7) % 32   # (284 with 31: length 258 without symbol 285)
        e = 8191 if j % 16 == 0 else 0 if j % 16 == 1 else (j * 2731) % 8192
        s.match(dc.LEN_BASE[sym - 257] + extra, (16385, 24577)[j % 2] + e, length_symbol=sym)

    def lit8():
        s.lit(n[0] % 250)
        n[0] += 1

    def lit9():
        s.lit(254)
        n[0] += 1

    def lit10():
        s.lit(255)
        n[0] += 1
    for _ in range(16):
        for _ in range(32):
            tok()
        lit9()
    while n[0] + 3 <= min(ntokens, 600):
        tok(), lit8(), lit10()
    while n[0] + 3 <= min(ntokens, 1110):
        tok(), tok(), lit9()
    while n[0] + 6 <= ntokens:
        tok(), lit8(), tok(), lit10(), tok(), lit9()
    s.eob()


def _craft_w1(s, dist, final, rnd):
    """dist non-periodic bytes stored, then a match of every length 3..258 at that distance, a literal behind every
    third: 33 408 bytes of matches whose starts and sources drift through every phase of the writer's rounds"""
    s.stored(rnd.randbytes(dist), False)
    s.fixed_block(final)
    for k, length in enumerate(range(3, 259)):
        s.match(length, dist)
        if k % 3 == 2:
            s.lit((k * 37 + 11) & 0xff)
    s.eob()


def _craft_chain(s, length, dist, n, final):
    """n matches, each one's source the match before it"""
    s.fixed_block(final)
    for i in range(dist):
        s.lit(0x41 + i)
    for _ in range(n):
        s.match(length, dist)
    s.eob()


def _craft_w3(s, nblocks, npairs, final):
    """rounds that run out of records before they run out of bytes: blocks of one literal, (literal, short match)
    pairs, and k = 0..5 literals before a match, before an end of block and before a stored block"""
    for i in range(nblocks):
        s.fixed_block(False)
        s.lit((i * 131 + 7) & 0xff)
        s.eob()
    s.fixed_block(False)
    for b in b"xyz":
        s.lit(b)
    for i in range(npairs):
        s.lit(i & 0xff)
        s.match(3, 3 + i % 2)
    s.eob()
    s.fixed_block(False)
    for rep in range(3):
        for k in range(6):
            for j in range(k):
                s.lit(0x30 + j + rep)
            s.match(4, 5)
    s.eob()
    for rep in range(3):
        for k in range(6):
            s.fixed_block(False)
            for j in range(k):
                s.lit(0x61 + j + rep)
            s.eob()
    for rep in range(3):
        for k in range(6):
            s.fixed_block(False)
            for j in range(k):
                s.lit(0x41 + j + rep)
            s.eob()
            s.stored(bytes([0x80 + k, 0x90 + rep, 0xa0]), False)
    s.fixed_block(final)
    s.lit(0x2e)
    s.eob()


def _craft_w4(op, kind, ok, variant, rnd):
    """op bytes in an earlier stored / fixed / dynamic block, then a match at distance op (ok) or op + 1"""
    s = dc.Stream()
    data = rnd.randbytes(op)
    if kind == "stored":
        s.stored(data, False)
    else:
        if kind == "fixed":
            s.fixed_block(False)
        else:
            s.dynamic_block(*_t1_code(), False)
        for b in data:
            s.lit(b)
        s.eob()
    s.fixed_block(True)
    length, sym = ((258, 285), (258, 284), (3, None))[variant]
    s.match(length, op if ok else op + 1, length_symbol=sym)
    s.lit(0x21)
    s.eob()
    return s


def _craft_data_block(s, final):
    s.fixed_block(final)
    for b in b"hello, hello":
        s.lit(b)
    s.match(5, 7)
    s.eob()


def _craft_b1(s, kind, n, final):
    """n empty blocks, then data.  Empty stored blocks: each behind a fixed block of 0..7 nine-bit literals, so that
    its header follows each of the 8 bit phases; the bits skipped up to the byte boundary are ones."""
    for i in range(n):
        if kind == "fixed":
            s.fixed_block(False)
            s.eob()
        elif kind == "dynamic":
            s.dynamic_block([0] * 256 + [1], [0], False)
            s.eob()
        else:
            s.fixed_block(False)
            for j in range((i - 2) % 8):
                s.lit(200 + j)
            s.eob()
            s.stored(b"", False, pad_bits=0xff)
    _craft_data_block(s, final)


def _craft_b2(s, final):
    """1024 blocks, alternately fixed and dynamic, a pair an odd number of bits long: 512 pairs put a header of either
    kind at every residue mod 512"""
    lit = [0] * 257
    lit[97] = lit[256] = 1

    def pair(t, extra):
        t.fixed_block(False)
        t.lit(200)
        if extra:
            t.lit(201)
        t.eob()
        t.dynamic_block(lit, [0], False)
        t.lit(97)
        t.eob()
    probe = dc.Stream()
    pair(probe, False)
    extra = probe.bitpos % 2 == 0
    for _ in range(512):
        pair(s, extra)
    _craft_data_block(s, final)


def _small_dyn(s, final, lit=None, dist=None, **plan):
    """a small complete code: literals a, b, c at 2 bits, end of block and length symbol 257 at 3; distances 1 and 2"""
    if lit is None:
        lit = [0] * 258
        lit[97] = lit[98] = lit[99] = 2
        lit[256] = lit[257] = 3
    if dist is None:
        dist = [1, 1]
    s.dynamic_block(lit, dist, final, plan or None)


def _craft_headers():
    """-> [(name, Stream)]: H1..H4"""
    out = []

    def new(name):
        s = dc.Stream()
        out.append((name, s))
        return s

    def abc(s, with_match=True):
        for b in b"abcabc":
            s.lit(b)
        if with_match:
            s.match(3, 2)
        s.eob()

    def garbage(s, status):
        s.raw_bits(0x2d5a, 16)
        s.raw_bits(0x1234, 16)
        s.expect_fail(status)
    # H1: field limits
    s = new("H1/hlit257")
    lit = [0] * 257
    lit[97] = lit[98] = lit[99] = lit[256] = 2
    s.dynamic_block(lit, [0], True)
    abc(s, False)
    s = new("H1/hlit286")
    lit = [0] * 286
    lit[97] = lit[98] = lit[99] = 2
    lit[256] = lit[285] = 3
    s.dynamic_block(lit, [1, 1], True)
    s.lit(97), s.lit(98), s.match(258, 1), s.match(258, 2), s.eob()
    for n in (287, 288):
        s = new("H1/hlit%d" % n)
        s.dynamic_block(lit + [0] * (n - 286), [1, 1], True)
        garbage(s, dc.INVALID_BUFFER)
    s = new("H1/hdist1")
    _small_dyn(s, True, dist=[1])
    s.lit(97), s.match(3, 1), s.eob()
    s = new("H1/hdist30")
    s.stored(bytes(range(256)) * 128, False)
    _small_dyn(s, True, dist=[1] + [0] * 28 + [1])
    s.lit(97), s.match(3, 32768), s.match(3, 1), s.match(3, 24577), s.eob()
    for n in (31, 32):
        s = new("H1/hdist%d" % n)
        _small_dyn(s, True, dist=[1] + [0] * (n - 2) + [1])
        garbage(s, dc.INVALID_BUFFER)
    s = new("H1/hclen4")   # only 16, 17, 18 and 0 can have a code: every length is zero, the first token has no code
    cl = [0] * 19
    cl[18] = cl[0] = 1
    s.dynamic_block([0] * 257, [0], True, {"symbols": [(18, 127), (18, 109)], "cl_lens": cl, "hclen": 4})
    garbage(s, dc.INVALID_BUFFER)
    s = new("H1/hclen19")
    s.dynamic_block(*_t1_code(), True)
    assert s.lit_lens[284] == 15
    for b in b"\x00\xfe\xff\x10":
        s.lit(b)
    s.match(258, 3, length_symbol=284), s.match(3, 4), s.eob()
    # H2: repeat symbols.  The lengths are what the symbols spell: literal 150 (151), the end of block, length symbol 257
    def spelled(name, symbols, hlit, hdist, tokens, status=None):
        s = new(name)
        lens = dc.expand_cl_symbols(symbols)
        if status is None:
            assert len(lens) == hlit + hdist
            s.dynamic_block(lens[:hlit], lens[hlit:], True, {"symbols": symbols})
            tokens(s)
        else:
            lens = (lens or []) + [0] * 320
            s.dynamic_block(lens[:hlit], lens[hlit:hlit + hdist], True, {"symbols": symbols, "check": False})
            garbage(s, status)
    zeros150 = [(18, 127), (18, 1)]
    after = [(17, 0), (16, 0), (18, 127), (16, 3)]   # 3 + 3 + 138 + 6 zeros: the 16s repeat a zero
    rest = [(2, 0)] * 3 + [(18, 92), (3, 0), (3, 0), (1, 0), (1, 0)]
    spelled("H2/16_first", [(16, 0)] + after + rest, 258, 2, None, dc.INVALID_BUFFER)
    spelled("H2/16_after_17_and_18", after + rest, 258, 2,
            lambda s: (s.lit(150), s.lit(151), s.lit(152), s.match(3, 2), s.eob()))
    spelled("H2/16_crosses_border", zeros150 + [(2, 0), (2, 0), (18, 93), (2, 0), (16, 2)], 258, 4,
            lambda s: (s.lit(150), s.lit(151), s.lit(150), s.lit(151), s.match(3, 4), s.match(3, 1), s.eob()))
    spelled("H2/18_crosses_border", zeros150 + [(1, 0), (18, 94), (1, 0), (18, 2), (1, 0), (1, 0)], 260, 12,
            lambda s: (s.lit(150), s.lit(150), s.eob()))
    tail = zeros150 + [(1, 0), (18, 94), (2, 0), (2, 0)]   # 150 at 1 bit, end of block and 257 at 2
    spelled("H2/16_ends_exactly", tail + [(2, 0), (16, 0)], 258, 4,
            lambda s: (s.lit(150), s.lit(150), s.lit(150), s.lit(150), s.match(3, 4), s.match(3, 1), s.eob()))
    spelled("H2/16_one_past", tail + [(2, 0), (16, 1)], 258, 4, None, dc.INVALID_BUFFER)
    spelled("H2/17_ends_exactly", tail + [(1, 0), (1, 0), (17, 0)], 258, 5,
            lambda s: (s.lit(150), s.lit(150), s.match(3, 2), s.eob()))
    spelled("H2/17_one_past", tail + [(1, 0), (1, 0), (17, 1)], 258, 5, None, dc.INVALID_BUFFER)
    s = new("H2/16_past_320")   # HLIT 286, HDIST 30: at place 315 a repeat of 6 would fill 321 places
    s.dynamic_block([0] * 286, [0] * 30, True,
                    {"symbols": [(18, 127), (18, 127), (17, 7)] + [(8, 0)] * 29 + [(16, 3)], "check": False})
    garbage(s, dc.INVALID_BUFFER)
    # H3: the code-length code itself
    one = [0] * 19
    one[9] = 1
    s = new("H3/single_symbol")   # 258 times "9": 257 + 1 codes of 9 bits, half the space of either alphabet unused
    s.dynamic_block([9] * 259, [9], True, {"symbols": [(9, 0)] * 260, "cl_lens": one})
    for b in b"single":
        s.lit(b)
    s.match(4, 1), s.eob()
    s = new("H3/single_symbol_unused_pattern")
    s.dynamic_block([9] * 257, [9], True, {"symbols": [(9, 0), (("raw", 1, 1), 0)] + [(9, 0)] * 256, "cl_lens": one, "check": False})
    garbage(s, dc.INVALID_SYMBOL)
    over = [0] * 19
    over[0] = over[8] = over[9] = 1
    s = new("H3/oversubscribed")
    s.dynamic_block([8] * 257, [9], True, {"symbols": [(0, 0)] * 5, "cl_lens": over, "check": False})
    garbage(s, dc.INVALID_BUFFER)
    s = new("H3/all_zero")
    s.dynamic_block([0] * 257, [0], True, {"symbols": [], "cl_lens": [0] * 19, "hclen": 4, "check": False})
    garbage(s, dc.INVALID_SYMBOL)
    # H4: the literal and distance code sets
    for n in range(1, 16):
        lens = list(range(1, n)) + [n, n, n]   # a complete set and one code more at length n
        for alphabet in ("lit", "dist"):
            s = new("H4/%s_oversubscribed_%d" % (alphabet, n))
            if alphabet == "lit":
                lit = [0] * 257
                lit[40:40 + len(lens)] = lens
                s.dynamic_block(lit, [1, 1], True)
            else:
                _small_dyn(s, True, dist=lens)
            garbage(s, dc.INVALID_BUFFER)
    s = new("H4/no_distance_code_literals_only")
    _small_dyn(s, True, dist=[0])
    abc(s, False)
    s = new("H4/no_distance_code_one_match")
    _small_dyn(s, True, dist=[0])
    s.lit(97), s.lit(98), s.lit(99)
    s.raw_code("lit", s.lit_codes[257], 3)
    garbage(s, dc.INVALID_BUFFER)
    s = new("H4/no_end_of_block_code")   # literals (the all-zero pattern is one) until the input runs out
    lit = [0] * 257
    lit[97] = 1
    lit[98] = lit[99] = 2
    s.dynamic_block(lit, [0], False)
    for b in b"abcabcaabbcc" * 5:
        s.lit(b)
    s.expect_fail(dc.END_OF_BUFFER)
    return out


def _craft_t2_t3():
    """-> [(name, Stream)]: unused patterns of incomplete codes (each followed by valid data) and the fixed codes'
    symbols without a meaning"""
    out = []

    def new(name):
        s = dc.Stream()
        out.append((name, s))
        return s

    def lit_set(lens_abc_eob_257):
        lit = [0] * 258
        lit[97], lit[98], lit[99], lit[256], lit[257] = lens_abc_eob_257
        return lit
    # literal/length codes: {a, b, EOB at 2 bits} leaves "11" unused (inside the root table); 1, 2, .., 12 bits leaves
    # twelve ones unused (beyond it)
    deep = [0] * 258
    for k in range(11):
        deep[97 + k] = k + 1
    deep[256] = 12
    for name, lit, pattern, nbits in (("lit_short", lit_set((2, 2, 0, 2, 0)), 0b11, 2), ("lit_long", deep, 0xfff, 12)):
        s = new("T2/%s_used" % name)
        s.dynamic_block(lit, [1, 1], True)
        for b in b"abbaabab" + (bytes(range(97, 108)) if name == "lit_long" else b""):
            s.lit(b)
        s.eob()
        s = new("T2/%s_unused" % name)
        s.dynamic_block(lit, [1, 1], True)
        s.lit(97), s.lit(98)
        s.raw_code("lit", pattern, nbits)
        s.expect_fail(dc.INVALID_BUFFER)
        for b in b"abab":
            s.lit(b)
        s.eob()
    # distance codes: {0, 1, 2 at 2 bits} leaves "11"; 1, 2, .., 10 bits leaves ten ones; a single code of one bit
    for name, dist, pattern, nbits in (("dist_short", [2, 2, 2], 0b11, 2), ("dist_long", list(range(1, 11)), 0x3ff, 10),
                                       ("dist_single", [1], 0b1, 1)):
        s = new("T2/%s_used" % name)
        _small_dyn(s, True, dist=dist)
        for b in b"abcabcabcabc":
            s.lit(b)
        for d in range(len(dist)):
            s.match(3, dc.DIST_BASE[d])
        s.eob()
        s = new("T2/%s_unused" % name)
        _small_dyn(s, True, dist=dist)
        for b in b"abcabcabcabc":
            s.lit(b)
        s.raw_code("lit", s.lit_codes[257], 3)
        s.raw_code("dist", pattern, nbits)
        s.expect_fail(dc.INVALID_BUFFER)
        for b in b"abc":
            s.lit(b)
        s.match(3, 1), s.eob()
    for sym in (286, 287):
        s = new("T3/fixed_litlen_%d" % sym)
        s.fixed_block(True)
        s.lit(1), s.lit(2), s.lit(3)
        s.raw_code("lit", s.lit_codes[sym], 8)
        s.expect_fail(dc.INVALID_BUFFER)
        s.raw_bits(0, 5), s.lit(4), s.eob()
    for sym in (30, 31):
        s = new("T3/fixed_dist_%d" % sym)
        s.fixed_block(True)
        s.lit(1), s.lit(2), s.lit(3)
        s.raw_code("lit", s.lit_codes[257], 7)
        s.raw_code("dist", sym, 5)
        s.expect_fail(dc.INVALID_BUFFER)
        s.lit(4), s.eob()
    return out


def _craft_b4():
    """-> [(name, Stream)]: the last end-of-block code followed by 0..7 padding bits (ones); input that ends inside a
    length's extra bits, inside a distance code and inside a stored block's LEN.  The cut streams' blocks are not
    final and their codes read zero bits as literals, so what the reference makes of the missing bits (it reads
    zeros) is decided by its end-of-buffer check alone."""
    out = []
    for pad in range(8):
        s = dc.Stream()
        s.fixed_block(True)
        s.lit(65)
        while (s.bitpos + 7 + pad) % 8:
            s.lit(200)   # nine bits: moves the phase by one
        s.eob()
        assert (8 - s.bitpos % 8) % 8 == pad
        s.final_pad = 0xff
        out.append(("B4/eob_pad_%d" % pad, s))
    lit = [0] * 282
    for i in range(97, 97 + 7):
        lit[i] = 3
    lit[256] = lit[281] = 4   # (281: five extra bits)
    for what in ("length_extra", "distance_code"):
        s = dc.Stream()
        s.dynamic_block(lit, [2, 2, 2, 2], False)
        for b in b"abcdefg":
            s.lit(b)
        while True:   # literals until the field straddles a byte border
            field = s.bitpos + 4 if what == "length_extra" else s.bitpos + 4 + 5
            width = 5 if what == "length_extra" else 2
            cut = (field // 8 + 1) * 8
            if field < cut < field + width:
                break
            s.lit(97)
        s.match(131 + 21, 3, length_symbol=281)
        s.cut_at_bit(cut)
        s.expect_fail(dc.END_OF_BUFFER)
        out.append(("B4/ends_in_" + what, s))
    s = dc.Stream()
    _craft_data_block(s, False)
    s.stored(b"never read", True)
    s.cut_at_bit((s.headers[-1][0] + 3 + 7) // 8 * 8 + 8)   # one byte of LEN and nothing behind it
    s.expect_fail(dc.INVALID_BUFFER)                        # LEN + NLEN (read as zero) is not 65535
    out.append(("B4/ends_in_stored_len", s))
    return out


W1_DISTANCES = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 258, 259, 2047, 2048, 2049, 4095, 4096, 4097,
                8191, 8192, 8193, 32767, 32768)
W1_DISTANCES_SMALL = (1, 3, 8, 259, 2048, 32768)
CRAFT_COUNTS = {"T1": 1, "T2": 10, "T3": 4, "W1": 30, "W2": 4, "W3": 1, "W4": 27, "B1": 12, "B2": 1, "B3": 1, "B4": 11,
                "H1": 10, "H2": 9, "H3": 4, "H4": 33}
CRAFT_COUNTS_SMALL = {"T1": 1, "T2": 10, "T3": 4, "W1": 6, "W2": 4, "W3": 1, "W4": 6, "B1": 3, "B2": 1, "B3": 1, "B4": 11,
                      "H1": 10, "H2": 9, "H3": 4, "H4": 33}
_craft_cache = {}


def crafted_streams(small=False, info=None):
    """The families T1-T3 (tokens), W1-W4 (writer), B1-B4 (blocks), H1-H4 (headers) -> [(name, raw deflate, plain or
    None, status or None)].  info: a dict that receives name -> (token positions, header positions) of the builder.
    small: the subset for the emulator (about 300 KB of output)."""
    if small not in _craft_cache:
        rnd = random.Random(1951)
        named = []

        def new(name):
            s = dc.Stream()
            named.append((name, s))
            return s
        _craft_t1(new("T1/48_bit_tokens"), 600 if small else 1500, True, rnd)
        named += _craft_t2_t3()
        for d in W1_DISTANCES_SMALL if small else W1_DISTANCES:
            _craft_w1(new("W1/dist_%d" % d), d, True, rnd)
        chains = 500 if small else 3000
        for length, d, n in ((3, 3, chains), (3, 1, chains), (4, 2, chains), (258, 1, 300 if small else 3000)):
            _craft_chain(new("W2/chain_len%d_dist%d" % (length, d)), length, d, n, True)
        _craft_w3(new("W3/starved_rounds"), 1500 if small else 9000, 500 if small else 3000, True)
        k = 0
        for op in (1, 2, 258, 32767, 32768):
            for kind in ("stored", "fixed", "dynamic"):
                for ok in (True, False):
                    k += 1
                    if not ok and op == 32768:
                        continue   # (32 769 is a distance the format cannot write)
                    if small and not (op, kind) in ((1, "fixed"), (258, "dynamic"), (32767, "stored")):
                        continue
                    named.append(("W4/op%d_%s_%s" % (op, kind, "at" if ok else "past"), _craft_w4(op, kind, ok, k % 3, rnd)))
        for kind in ("fixed", "dynamic", "stored"):
            for n in (52,) if small else (1, 51, 52, 5000):
                _craft_b1(new("B1/%d_empty_%s" % (n, kind)), kind, n, True)
        _craft_b2(new("B2/header_at_every_residue"), True)
        text = synth.corpus_file("alice29.txt")[:5000 if small else 20000]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        parts = []
        for o in range(0, len(text), 50):
            parts.append(c.compress(text[o:o + 50]))
            parts.append(c.flush(zlib.Z_PARTIAL_FLUSH))
        parts.append(c.flush())
        named += _craft_b4()
        named += _craft_headers()
        cases, positions = [], {}
        for name, s in named:
            positions[name] = (s.tokens, s.headers)
            cases.append((name,) + s.finish())
        cases.append(("B3/partial_flush_every_50", b"".join(parts), text, None))
        _craft_cache[small] = (cases, positions)
    cases, positions = _craft_cache[small]
    if info is not None:
        info.update(positions)
    return list(cases)


def crafted_coverage(positions):
    """the coverage conditions of T1 and B2, from the builder's positions: (residues mod 512 at which a 48-bit token
    starts, residues at which a fixed block's header starts, residues at which a dynamic block's does)"""
    tokens, _ = positions["T1/48_bit_tokens"]
    _, headers = positions["B2/header_at_every_residue"]
    return ({p % 512 for p, bits, kind in tokens if kind == "match" and bits == 48},
            {p % 512 for p, btype in headers if btype == 1}, {p % 512 for p, btype in headers if btype == 2})


# Rejected cases whose status is not compared with the oracle's, only that both refuse: name -> reason
CRAFT_STATUS_EXCEPTIONS = {}
CRAFT_SINGLE_FAMILIES = ("T1", "W2", "W3", "B1")


def _stderr_of(fn):
    """fn() with file descriptor 2 in a temporary file -> (result, what the library wrote there)"""
    import sys
    import tempfile
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            res = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return res, tmp.read().decode("utf-8", "replace")


def check_crafted_streams(eng, small=False):
    """crafted_streams() through the device decoder: all of them in one batch (expected bytes, the oracle's status for
    every rejected one, neighbours untouched); T1 / W2 / W3 / B1 again one stream a call (the wide kernels); the
    accepted ones wrapped as gzip and zlib through dfDetect (the checksum kernels see this output too); into slots of
    exactly the expected size and one byte short (ZH_ERR_DST_TOO_SMALL with the true length, the bytes between the
    slots unchanged); and the sizing pass for the stream that outgrows the guess a raw stream gets."""
    cases = crafted_streams(small)
    outs, sts = eng.uncompress_batch([c[1] for c in cases], oracle.dfDeflate)
    bad = []
    for (name, blob, plain, status), got, st in zip(cases, outs, sts):
        if plain is not None:
            if st != 0 or got != plain:
                bad.append((name, st, None if got is None else len(got), len(plain)))
        elif st == 0 or (st != status and name not in CRAFT_STATUS_EXCEPTIONS):
            bad.append((name, "status", st, "expected", status))
    assert not bad, bad
    for name, blob, plain, status in cases:
        if name.split("/")[0] in CRAFT_SINGLE_FAMILIES:
            got, st = eng.uncompress_batch([blob], oracle.dfDeflate)
            assert st == [0] and got[0] == plain, (name, "alone", st)
    good = [c for c in cases if c[2] is not None]
    wrapped = []
    for name, blob, plain, _ in good:
        wrapped.append(b"\x1f\x8b\x08\x00" + b"\x00" * 6 + blob + struct.pack("<II", zlib.crc32(plain), len(plain)))
        wrapped.append(b"\x78\x9c" + blob + struct.pack(">I", zlib.adler32(plain)))
    outs, sts = eng.uncompress_batch(wrapped, oracle.dfDetect)
    bad = [(good[i // 2][0], ("gzip", "zlib")[i % 2], sts[i]) for i in range(len(wrapped))
           if sts[i] != 0 or outs[i] != good[i // 2][2]]
    assert not bad, bad
    hurt = bytearray(wrapped[0])
    hurt[-5] ^= 0x10   # (the premise: a wrong checksum does not pass)
    assert eng.uncompress_batch([bytes(hurt)], oracle.dfDetect)[1] == [ZH_ERR_CHECKSUM]
    for short in (0, 1):
        some = [c for c in good if len(c[2]) >= short]
        caps = [len(c[2]) - short if c[2] else 0 for c in some]
        offs, pos = [], 5
        for c in caps:
            offs.append(pos)
            pos += c + 7
        arena = bytearray(b"\xa5" * (pos + 16))
        view = memoryview(arena)
        lens, sts, filled = eng.uncompress_batch_into([c[1] for c in some], [view[o:o + c] for o, c in zip(offs, caps)],
                                                      oracle.dfDeflate)
        keep = bytearray(b"\x01" * len(arena))
        for (name, blob, plain, _), o, c, ln, st in zip(some, offs, caps, lens, sts):
            assert ln == len(plain), (name, short, ln, len(plain))
            if c == len(plain):
                assert st == 0 and bytes(arena[o:o + c]) == plain, (name, short, st)
            else:
                assert st == ZH_ERR_DST_TOO_SMALL, (name, short, st)
            keep[o:o + c] = bytes(c)
        changed = [i for i in range(len(arena)) if keep[i] and arena[i] != 0xa5]
        assert not changed, ("bytes outside the slots changed", short, changed[:4])
    # raw deflate gets 4 x its size + 64 KiB: the chains of short matches stay below that, the chain of 258-byte
    # matches does not -- decode, count, decode again
    by_name = {c[0]: c for c in cases}
    old = os.environ.get("ZH_TRACE")
    os.environ["ZH_TRACE"] = "1"
    try:
        for name, passes in (("W2/chain_len258_dist1", 3), ("W2/chain_len3_dist3", 1)):
            blob, plain = by_name[name][1:3]
            assert (len(plain) > 4 * len(blob) + 65536) == (passes == 3)
            (got, st), err = _stderr_of(lambda: eng.uncompress_batch([blob], oracle.dfDeflate))
            assert st == [0] and got[0] == plain
            assert err.count("uncompress: kernels") == passes, (name, err)
    finally:
        if old is None:
            del os.environ["ZH_TRACE"]
        else:
            os.environ["ZH_TRACE"] = old


def crafted_segment_streams(small=False):
    """Crafted blocks back to back in one stream, only the last block final: a stored preamble, W1 at distances
    32 768 and 32 767, the W2 chains, T1, 52 empty blocks of each kind, then text in zlib's dynamic blocks.  The same
    with a symbol that has no meaning (fixed code 286) late in the text, and with a distance one beyond the start of
    the output early (the format cannot write such a distance once 32 768 bytes are out).
    -> [(raw deflate, plain or None, status or None)]"""
    text = synth.gen_batch("text", 1, 120000 if small else 600000, first_index=4)[0].tobytes()
    out = []
    for fault in (None, "late", "early"):
        rnd = random.Random(32768)
        s = dc.Stream()
        s.stored(rnd.randbytes(1000), False)
        if fault == "early":
            s.fixed_block(False)
            s.lit(1), s.match(3, 1002), s.eob()
        s.stored(rnd.randbytes(30000), False)
        _craft_w1(s, 32768, False, rnd)
        _craft_w1(s, 32767, False, rnd)
        for length, d in ((3, 3), (3, 1), (4, 2)):
            _craft_chain(s, length, d, 500 if small else 3000, False)
        _craft_t1(s, 600 if small else 1500, False, rnd)
        for kind in ("fixed", "dynamic", "stored"):
            _craft_b1(s, kind, 52, False)
        s.stored(b"", False)   # (byte-aligned from here on: zlib's blocks end in stored ones, which do not shift)
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        step = len(text) // 6
        for k in range(6):
            part = text[k * step:(k + 1) * step]
            s.append_bytes(c.compress(part) + c.flush(zlib.Z_FULL_FLUSH), part)
            if fault == "late" and k == 4:
                s.fixed_block(False)
                s.lit(2)
                s.raw_code("lit", s.lit_codes[286], 8)
                s.expect_fail(dc.INVALID_BUFFER)
                s.lit(3), s.eob()
                s.stored(b"", False)
        s.append_bytes(c.flush(), b"")
        out.append(s.finish())
    return out


def check_crafted_segmented(eng, monkeypatch, small=False):
    """The streams above decoded segment-wise (2 048-byte segments): the expected bytes, the stream was cut, and the
    faulty streams end with the status the one-workgroup decode gives them -- the oracle's."""
    monkeypatch.setenv("ZH_SEG_MIN", "8192")
    monkeypatch.setenv("ZH_SEG_BYTES", "2048")
    monkeypatch.setenv("ZH_SEG_SETUP", "0")
    for blob, plain, status in crafted_segment_streams(small):
        try:
            ref = oracle.uncompress(blob, oracle.dfDeflate)
            assert plain is not None and ref == plain
        except oracle.ZippyError as e:
            assert plain is None and e.status == status
        before = eng.segment_stats()
        outs, sts = eng.uncompress_batch([blob], oracle.dfDeflate)
        cut = eng.segment_stats()[0] - before[0]
        assert cut >= 1, "the stream was not cut into segments"
        if plain is not None:
            assert sts == [0] and outs[0] == plain, sts
        else:
            monkeypatch.setenv("ZH_SEG", "0")
            _, whole = eng.uncompress_batch([blob], oracle.dfDeflate)
            monkeypatch.setenv("ZH_SEG", "1")
            assert sts == whole == [status], (sts, whole, status)
    for k in ("ZH_SEG_MIN", "ZH_SEG_BYTES", "ZH_SEG_SETUP", "ZH_SEG"):
        monkeypatch.delenv(k, raising=False)


# ---- crafted compress inputs: the encoder at its decision thresholds (stored / fixed / dynamic, the code lengths'
# run-length coding, emission at its widest, the BestSpeed matcher's edges) ----
FULL_BLOCK = 4194304
FRAG = 32768
S_LEN_FIRST = 267501   # the first block length at which the float32 product and len * 98 // 100 disagree
S_LEN_SECOND = 600001  # (another one below 1 MiB)
F_LENGTHS = (0, 1, 2, 3, 4, 5, 6, 14, 15, 16, 2047, 2048, 2049)
ALL_LEVELS = (-2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9)
CHAIN_LEVELS = (2, 4, 6, 9)
GZIP_ONLY = (oracle.dfGzip,)
CLCL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
R_ZERO_RUNS = (1, 2, 3, 4, 10, 11, 12, 137, 138, 139, 140, 141, 148, 149, 150, 255)
R_NONZERO_RUNS = tuple(range(1, 14)) + (19,)
R_HEADS = (0, 63, 64, 127, 128, 191, 192, 255, 256)


def stored_threshold(n):
    """deflate.nim:274-277: a block of n bytes is stored from this many literals on -- a float32 product, truncated"""
    return int(np.float32(n) * np.float32(0.98))


def token_matches(toks):
    """the reference's u16 token stream -> ([(position in the block, offset, length)], bytes covered)"""
    out, pos, i = [], 0, 0
    toks = [int(t) for t in toks]
    while i < len(toks):
        if toks[i] & 0x8000:
            out.append((pos, toks[i + 1], toks[i + 2]))
            pos += toks[i + 2]
            i += 3
        else:
            pos += toks[i]
            i += 1
    return out, pos


def _s_input(noise, k, total, tail):
    """k bytes of noise, then a run of one byte up to `total`, then the second block's bytes"""
    return noise[:k] + b"\x5a" * (total - k) + tail


def _s_find(noise, total, tail, level, target):
    """the input of _s_input whose first block has exactly `target` literals (the count grows by about one a byte of
    noise; where it jumps over the target, a short island of noise inside the run makes up the difference)"""
    block = min(total, FULL_BLOCK)
    k, seen = target, {}
    for _ in range(48):
        k = max(0, min(total, k))
        if k in seen:
            break
        got = oracle.block_tokens(_s_input(noise, k, total, tail), level, 0, block)[3]
        if got == target:
            return _s_input(noise, k, total, tail)
        seen[k] = got
        k += target - got
    below = [kk for kk, g in seen.items() if g < target]
    if below:
        k = max(below, key=lambda kk: seen[kk])
        for island in range(1, 64):  # noise bytes in the middle of the run: a few more literals
            src = bytearray(_s_input(noise, k, total, tail))
            at = k + (total - k) // 2
            src[at:at + island] = noise[-island:]
            if oracle.block_tokens(bytes(src), level, 0, block)[3] == target:
                return bytes(src)
    return None


def _s_cases(small):
    rnd = random.Random(9801)
    noise = rnd.randbytes(FULL_BLOCK)
    text = synth.corpus_file("alice29.txt")[3000:4000]
    tail_noise = rnd.randbytes(1000)
    out = []
    for level, total in ((1, S_LEN_FIRST), (-1, S_LEN_FIRST), (1, S_LEN_SECOND)):
        if small and (level, total) != (1, S_LEN_FIRST):
            continue
        t = stored_threshold(total)
        for target in sorted({t - 1, t, t + 1, total * 98 // 100}):
            out.append(("S/len%d_level%d_nlit%d" % (total, level, target), _s_find(noise, total, b"", level, target),
                        (level,), GZIP_ONLY))
    if not small:
        t = stored_threshold(FULL_BLOCK)
        for level in (1, 9):
            for target, tail, kind in ((t - 1, text, "text"), (t - 1, tail_noise, "noise"), (t, text, "text"),
                                       (t, tail_noise, "noise"), (t + 1, text, "text")):
                out.append(("S/full_level%d_nlit%d_then_%s" % (level, target, kind),
                            _s_find(noise, FULL_BLOCK, tail, level, target), (level,), GZIP_ONLY))
    return out


def f_inputs():
    """Family F: the tiny blocks and the fixed / dynamic border, three kinds of data -> [(name, bytes)]"""
    text = synth.corpus_file("alice29.txt")[5000:]
    out = []
    for n in F_LENGTHS:
        out.append(("F/text_%d" % n, text[:n]))
        out.append(("F/one_byte_%d" % n, b"\xe7" * n))
        out.append(("F/all_bytes_%d" % n, (bytes(range(256)) * 9)[:n]))
    return out


def _f_cases(small):
    out = []
    for name, src in f_inputs():
        if small and not name.endswith(("_0", "_3", "_15", "_2048", "_2049")):
            continue
        out.append((name, src, (1, 6, 7, 9), FORMATS))
        out.append((name + "/gzip", src, (-1,) if small else (-2, -1, 0, 2, 3, 4, 5, 8), GZIP_ONLY))
    return out


def dyadic_input(layout, top, seed):
    """Family R's builder.  layout: items laid over the byte values from 0 on -- ("z", n): n unused values;
    ("zto", p): unused values up to value p; ("n", n, l): n values of code length l; ("F",): the fill, single values
    of distinct lengths that bring the Kraft sum to exactly 1 with the end-of-block symbol at length `top`.  A value
    of length l occurs 2 ** (top - l) times: the histogram is dyadic, its Huffman lengths are the chosen ones.
    -> (shuffled bytes, {value: length})"""
    mass = sum(it[1] << (top - it[2]) for it in layout if it[0] == "n")
    deficit = (1 << top) - 1 - mass
    assert deficit >= 0, "layout too heavy"
    fill = [top - b for b in range(top - 1, -1, -1) if deficit >> b & 1]
    lens, pos = {}, 0
    for it in layout:
        if it[0] == "z":
            pos += it[1]
        elif it[0] == "zto":
            assert pos <= it[1], (pos, it)
            pos = it[1]
        elif it[0] == "n":
            for _ in range(it[1]):
                lens[pos] = it[2]
                pos += 1
        else:
            assert deficit >= 0 and fill is not None
            for l in fill:
                lens[pos] = l
                pos += 1
            fill = None
    assert pos <= 256 and (fill is None or not fill), (pos, fill)
    body = bytearray()
    for v, l in lens.items():
        body += bytes([v]) * (1 << (top - l))
    body = list(body)
    random.Random(seed).shuffle(body)
    return bytes(body), lens


def r_layouts():
    """name -> (layout, length of the end-of-block symbol)"""
    sep = lambda k: ("n", 1, 8 + k % 2)
    small_zero, k = [("F",)], 0
    for z in (1, 2, 3, 4, 10, 11, 12):
        small_zero += [("z", z), sep(k)]
        k += 1
    nonzero = [("F",), ("z", 1)]
    for k, n in enumerate((2, 3, 4, 5, 6, 7, 8)):
        nonzero += [("n", n, 9 + k % 2), ("z", 1 + k % 2)]
    nonzero2 = [("F",), ("z", 2)]
    for k, n in enumerate((9, 10, 11, 12, 13, 19)):
        nonzero2 += [("n", n, 9 + k % 2), ("z", 1)]
    out = {
        "small_zero_runs": (small_zero, 12),
        "nonzero_runs_2_8": (nonzero, 12),
        "nonzero_runs_9_19": (nonzero2, 12),
        # a run of 150 equal lengths over the whole second group of 64, heads in lanes 63 and 0
        "nonzero_run_150": ([("F",), ("zto", 40), ("n", 150, 9), ("z", 1), ("n", 1, 8)], 12),
        "nonzero_run_130_from_63": ([("F",), ("zto", 63), ("n", 130, 9)], 12),
        "nonzero_run_134": ([("F",), ("zto", 14), ("n", 134, 9), ("z", 2), ("n", 100, 10)], 13),
        # heads at 63 / 64, 127 / 128, 191 / 192, 255 / 256
        "heads_at_group_borders": ([("F",), ("zto", 63), ("n", 1, 8), ("zto", 127), ("n", 1, 8), ("zto", 191), ("n", 1, 8),
                                    ("zto", 255), ("n", 1, 8)], 12),
        "heads_nonzero_at_group_borders": ([("F",), ("zto", 60), ("n", 3, 9), ("n", 1, 8), ("n", 63, 9), ("n", 1, 8),
                                            ("n", 63, 10), ("n", 1, 8), ("n", 63, 9), ("n", 1, 8)], 13),
        "zero_137_from_63": ([("F",), ("zto", 62), ("n", 1, 8), ("z", 137), ("n", 1, 8)], 12),
        "zero_138_from_64": ([("F",), ("zto", 63), ("n", 1, 8), ("z", 138), ("n", 1, 8)], 12),
        "zero_139_from_0": ([("z", 139), ("F",)], 12),
        "zero_140_from_1": ([("n", 1, 8), ("z", 140), ("F",)], 12),
        "zero_141_to_191": ([("F",), ("zto", 49), ("n", 1, 8), ("z", 141), ("n", 1, 8), ("n", 1, 9)], 12),
        "zero_148_to_255": ([("F",), ("zto", 106), ("n", 1, 8), ("z", 148), ("n", 1, 8)], 12),
        "zero_149_to_192": ([("F",), ("zto", 42), ("n", 1, 8), ("z", 149), ("n", 1, 8)], 12),
        "zero_150": ([("F",), ("zto", 100), ("n", 1, 8), ("z", 150), ("n", 1, 8)], 12),
        # lengths up to 15 in the header: HCLEN + 4 = 19
        "length_15": ([("F",), ("z", 3), ("n", 5, 15), ("z", 4), ("n", 7, 14), ("zto", 250), ("n", 4, 15)], 15),
    }
    return out


def _r_cases(small):
    out = []
    for name, (layout, top) in r_layouts().items():
        src, _ = dyadic_input(layout, top, 77)
        out.append(("R/" + name, src, (-2,), FORMATS if name == "small_zero_runs" else GZIP_ONLY))
    # one used byte value: the longest run of zeros there is; the end-of-block symbol has length 1
    out.append(("R/zero_255", b"\xff" * 3000, (-2,), GZIP_ONLY))
    out.append(("R/zero_100_155", b"\x64" * 3000, (-2,), GZIP_ONLY))
    # with matches the lengths cannot be dictated: the oracle says what these reach (tests/test_compress_craft.py)
    rnd = random.Random(286)
    far = rnd.randbytes(1500)
    text = synth.corpus_file("alice29.txt")
    for level in (1, 9):
        out.append(("R/far_258_level%d" % level, far + text[:25000] + far + text[25000:26000], (level,), GZIP_ONLY))
    out.append(("R/period_3", b"abc" * 1000, (1, 9), GZIP_ONLY))
    out.append(("R/period_3_then_4", b"abc" * 700 + b"wxyz" * 700, (1, 9), GZIP_ONLY))  # the last run: two equal lengths
    for n in (2500, 2600, 3000, 5000):
        out.append(("R/run_%d" % n, b"\x11" * n, (1,), GZIP_ONLY))
    out.append(("R/text_8000", text[40000:48000], (1, 9), GZIP_ONLY))
    # eight periods, eight distance codes used alike: the distance lengths are 3 eight times, the last run of the array
    periods = b"".join((rnd.randbytes(p) * 2600)[:2600] for p in (1, 2, 3, 4, 5, 7, 9, 13))
    out.append(("R/eight_periods", periods, (1, 9), GZIP_ONLY))
    return out


def header_cells(src, level):
    """What the first block's dynamic header is made of, from the oracle alone: the maximal runs of the concatenated
    code lengths [(start, value, length)], n_litlen, n_dist and HCLEN + 4 (these three read back from the stream)."""
    block = min(len(src), FULL_BLOCK)
    _, lf, df, _ = oracle.block_tokens(src, level, 0, block)
    lit = list(oracle.huffman_codes(lf, 257, 15)[1])
    dist = list(oracle.huffman_codes(df, 2, 15)[1])
    arr = [int(x) for x in lit + dist]
    runs, i = [], 0
    while i < len(arr):
        j = i
        while j + 1 < len(arr) and arr[j + 1] == arr[i]:
            j += 1
        runs.append((i, arr[i], j - i + 1))
        i = j + 1
    head = int.from_bytes(oracle.compress(src, level, oracle.dfDeflate)[:4], "little")
    assert (head >> 1) & 3 == 2, "not a dynamic block"
    n_litlen, n_dist, hclen4 = ((head >> 3) & 31) + 257, ((head >> 8) & 31) + 1, ((head >> 13) & 15) + 4
    assert (n_litlen, n_dist) == (len(lit), len(dist))
    stream = int.from_bytes(oracle.compress(src, level, oracle.dfDeflate)[:16], "little")
    cl_lens = {sym: (stream >> (17 + 3 * k)) & 7 for k, sym in enumerate(CLCL_ORDER[:hclen4])}
    return {"runs": runs, "n_litlen": n_litlen, "n_dist": n_dist, "hclen4": hclen4, "lens": arr, "cl_lens": cl_lens}


E_RARE = tuple(range(40, 240))   # the rare byte values of E/long_literal_codes
E_FIRST_AT = 1077                # (no multiple of 512)
E_SECOND_AT = 3 * FRAG - 700     # the second stretch straddles a 32 KiB fragment border


def _e_cases(small):
    """Long literal codes: eleven dominant byte values whose frequencies double from 150 on, 200 rare values of 16
    occurrences below them -- a Huffman tree of depth 16, so the reference's length limit runs and lifts one rare
    value to 13 bits; the other 199, all of 14 or 15 bits, are laid out eight times each, shuffled, as a stretch of
    1 592 consecutive positions, and that stretch is placed twice.
    Long match tokens: long_match_input(), the same bytes at level 1 and at level 9."""
    rnd = random.Random(15)
    freq = np.zeros(286, np.uint32)
    for k in range(11):
        freq[1 + k] = 150 << k
    freq[list(E_RARE)] = 16
    freq[256] = 1
    lens = oracle.huffman_codes(freq, 257, 15)[1]
    wide = [v for v in E_RARE if lens[v] >= 14]
    stretch = []
    for _ in range(8):
        rnd.shuffle(wide)
        stretch += wide
    body = [v for v in E_RARE if lens[v] < 14] * 16
    for k in range(11):
        body += [1 + k] * (150 << k)
    rnd.shuffle(body)
    src = bytes(body[:E_FIRST_AT]) + bytes(stretch) + bytes(body[E_FIRST_AT:])
    src = src[:E_SECOND_AT] + bytes(stretch) + src[E_SECOND_AT:]
    wide_matches = long_match_input()
    return [("E/long_literal_codes", src, (-2,), FORMATS),
            ("E/long_match_tokens_level1", wide_matches, (1,), GZIP_ONLY),
            ("E/long_match_tokens_level9", wide_matches, (9,), GZIP_ONLY)]


E_LENGTH_LADDER = ((240, 16), (180, 32), (150, 64), (120, 128), (105, 256), (90, 512))   # (match length, how many)


def long_match_input():
    """Match tokens of 41 bits back to back.  The first fragment: 1 500 bytes of noise, noise up to 16 500, a run of
    200 equal bytes, then twelve pieces of 200 bytes of the first noise, each a match of its own (length symbol 283:
    5 extra bits; distance 16 385 or more: 13 extra bits).  At level 1 a piece starts where the matcher probed the
    noise (its stride grows by one every 32 misses), so the table still holds the place, and the run in front ends in
    a match, so the next candidate is looked up at the piece's first byte.  Behind it 300 000 bytes of short copies
    from near by, one fresh byte between two, so that far distances are rare among the distances; and among them
    long copies from near by whose counts double from one length symbol to the next (E_LENGTH_LADDER), a ladder
    with symbol 283 at its foot."""
    rnd = random.Random(1)
    noise = rnd.randbytes(1500)
    probes, at, skip = [], 1, 32
    while at < 1500 - 200:
        if at >= 8:
            probes.append(at)
        at += skip >> 5
        skip += 1
    frag = noise + rnd.randbytes(15000) + b"Z" * 200
    for start in sorted(rnd.sample(probes, 12), reverse=True):   # (descending: no piece continues the one before)
        frag += noise[start:start + 200]
    frag += rnd.randbytes(FRAG - len(frag))
    longs = [length for length, count in E_LENGTH_LADDER for _ in range(count)]
    rnd.shuffle(longs)
    every = (300000 - 120000) // 9 // len(longs)
    out, k = bytearray(rnd.randbytes(400)), 0
    while len(out) < 300000:
        k += 1
        if longs and k % every == 0:
            length = longs.pop()
            dist = length + 40
        else:
            dist, length = min(len(out), 1 + int(rnd.expovariate(1 / 60.0))), rnd.randrange(4, 9)
        for _ in range(length):
            out.append(out[-dist])
        out.append(rnd.randrange(256))
    assert not longs
    return frag + bytes(out[:300000])


LENGTH_BASES = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
DISTANCE_BASES = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
                  6145, 8193, 12289, 16385, 24577)


def widest_match_stretch(src, level, min_bits=40):
    """From the oracle's tokens and code lengths of the first block: the longest stretch of matches back to back (each
    starts where the one before ends) whose tokens -- length code, its extra bits, distance code, its extra bits --
    all have at least min_bits bits -> (positions covered, tokens, the fewest bits among them)"""
    toks, lf, df, _ = oracle.block_tokens(src, level, 0, min(len(src), FULL_BLOCK))
    lit = oracle.huffman_codes(lf, 257, 15)[1]
    dist = oracle.huffman_codes(df, 2, 15)[1]
    best, run = (0, 0, 0), []
    for pos, offset, length in token_matches(toks)[0]:
        lc = max(i for i, b in enumerate(LENGTH_BASES) if b <= length)
        dc = max(i for i, b in enumerate(DISTANCE_BASES) if b <= offset)
        bits = int(lit[257 + lc]) + (0 if lc < 8 or lc == 28 else (lc - 4) // 4) + int(dist[dc]) + max(0, dc // 2 - 1)
        if bits < min_bits:
            run = []
            continue
        if run and run[-1][0] + run[-1][1] != pos:
            run = []
        run.append((pos, length, bits))
        span = run[-1][0] + run[-1][1] - run[0][0]
        if span > best[0]:
            best = (span, len(run), min(r[2] for r in run))
    return best


M_TABLE_BORDERS = tuple(n + d for n in (256, 512, 1024, 2048, 4096, 8192, 16384) for d in (-1, 0, 1)) + (32767, 32768)


def _m_cases(small):
    """Family M: the BestSpeed matcher's edges -- fragment lengths at the table-size borders, tails shorter than 15
    bytes, position 0 as a candidate, chains of 258-byte matches and where they end, the growing probe stride, a
    fragment written twice."""
    rnd = random.Random(1415)
    html = synth.corpus_file("html")
    alice = synth.corpus_file("alice29.txt")
    runs = synth.gen_batch("runs", 1, 3 * FRAG + 70000, first_index=3)[0].tobytes()
    noise = rnd.randbytes(2 * FRAG + 40000)
    out = []

    def add(name, src, keep=True):
        if keep or not small:
            out.append(("M/" + name, src, (1,), GZIP_ONLY))
    for i, n in enumerate(M_TABLE_BORDERS):
        p, q = i % 3, (i + 1) % 3
        add("frag_%d_text_behind_%d" % (n, p), html[i * 100:i * 100 + p * FRAG + n], n in (255, 257, 4096, 16385))
        add("frag_%d_runs_behind_%d" % (n, q), runs[i * 64:i * 64 + q * FRAG + n], n in (256, 1025, 16384))
    for k in range(1, 17):
        add("tail_%d_behind_1" % k, (alice if k % 2 else runs)[k * 50:k * 50 + FRAG + k], k in (1, 14, 15, 16))
        add("tail_%d_behind_2" % k, (runs if k % 2 else html)[k * 70:k * 70 + 2 * FRAG + k], k in (2, 15))
    # the fragment's first four bytes again, at a place whose hash slot is still empty: candidate 0
    again = b"QRST-first-bytes" + noise[:14] + b"QRST-first-bytes" + alice[:500]
    add("position_0_first_fragment", again)
    add("position_0_later_fragment", html[:FRAG] + again)
    add("run_one_byte_fragment", b"\x07" * FRAG)
    add("run_period_2_fragment", b"\x07\x70" * (FRAG // 2), False)
    add("run_one_byte_two_fragments", b"\x33" * (2 * FRAG), False)
    for gap in (0, 14, 15, 16):   # a run up to `gap` bytes before the fragment's end
        add("run_ends_%d_before_end" % gap, noise[:20000] + b"\x21" * (FRAG - 20000 - gap) + noise[50000:50000 + gap] + alice[:3000],
            gap in (0, 15))
    add("run_crosses_border", alice[:FRAG - 1000] + b"\x42" * 2000 + alice[:4000])
    add("probe_stride", noise[:40000] + alice[:30000] + noise[40000:70000], False)
    add("fragment_twice", html[1000:1000 + FRAG] * 2, False)
    return out


_compress_craft_cache = {}


def crafted_inputs(small=False):
    """The families S (stored or not), F (fixed or dynamic, tiny blocks), R (the code lengths' run-length coding),
    E (emission at its widest) and M (the BestSpeed matcher's edges) -> [(name, bytes, levels, formats)].  What each
    input reaches is asserted from the oracle alone in tests/test_compress_craft.py.  small: the emulator's subset."""
    if small not in _compress_craft_cache:
        cases = _s_cases(small) + _f_cases(small) + _r_cases(small) + _e_cases(small) + _m_cases(small)
        assert len({c[0] for c in cases}) == len(cases)
        _compress_craft_cache[small] = cases
    return list(_compress_craft_cache[small])


_oracle_stream_cache = {}


def oracle_stream(name, src, level, fmt):
    """oracle.compress of a crafted input, computed once a process"""
    key = (name, level, fmt)
    if key not in _oracle_stream_cache:
        _oracle_stream_cache[key] = oracle.compress(src, level, fmt, fname_len=0)
    return _oracle_stream_cache[key]


def first_bit_difference(a, b):
    for i in range(min(len(a), len(b))):
        if a[i] != b[i]:
            x = a[i] ^ b[i]
            return 8 * i + (x & -x).bit_length() - 1
    return 8 * min(len(a), len(b))


def check_crafted_compress(eng, cases, levels=None):
    """check_compress_identical's conditions for named cases, one batch a (level, container): the device's bytes are
    the oracle's -- a mismatch names the case and the first bit that differs --, zlib and the oracle's uncompress give
    the input back, and so does the device's own.  levels: run every case at these instead of its own."""
    eng.set_gzip_fname_len(0)
    groups = {}
    for name, src, own, formats in cases:
        for level in (levels if levels is not None else own):
            for fmt in formats:
                groups.setdefault((level, fmt), []).append((name, src))
    bad = []
    for (level, fmt), items in groups.items():
        outs, sts = eng.compress_batch([s for _, s in items], level, fmt)
        for (name, src), out, st in zip(items, outs, sts):
            if st != 0:
                bad.append((name, level, fmt, "status", st))
                continue
            ref = oracle_stream(name, src, level, fmt)
            if out != ref:
                bad.append((name, level, fmt, "first differing bit", first_bit_difference(out, ref), "device %d B, oracle %d B"
                            % (len(out), len(ref))))
                continue
            assert zlib.decompress(out, WBITS[fmt]) == src, (name, level, fmt, "zlib")
            assert oracle.uncompress(out, fmt) == src, (name, level, fmt, "oracle.uncompress")
        good = [i for i, st in enumerate(sts) if st == 0]
        back, bsts = eng.uncompress_batch([outs[i] for i in good], fmt)
        for i, got, st in zip(good, back, bsts):
            if st != 0 or got != items[i][1]:
                bad.append((items[i][0], level, fmt, "device uncompress", st))
    assert not bad, bad


def check_crafted_contract(eng, cases, margin=1.02):
    """the same inputs under the opt-in parallel parse at level 1: valid streams that zlib and the oracle decode to
    the input (the header writer is shared with contract mode); margin: the batch's size against the oracle's, as
    check_parallel_parse takes it (None: not compared) -> (device bytes, oracle bytes)"""
    eng.set_gzip_fname_len(0)
    eng.set_l1_parse(1)
    try:
        outs, sts = eng.compress_batch([c[1] for c in cases], 1, oracle.dfGzip)
    finally:
        eng.set_l1_parse(-1)
    dev = ref = 0
    for (name, src, _, _), out, st in zip(cases, outs, sts):
        assert st == 0, (name, st)
        assert zlib.decompress(out, 31) == src, (name, "zlib")
        assert oracle.uncompress(out, oracle.dfGzip) == src, (name, "oracle.uncompress")
        dev += len(out)
        ref += len(oracle_stream(name, src, 1, oracle.dfGzip))
    if margin is not None:
        assert dev <= margin * ref, "parallel parse: %d B against the oracle's %d B" % (dev, ref)
    return dev, ref


def block_types(src, level):
    """BTYPE of every deflate block the oracle writes for src (a stored block of more than 65 535 bytes counts once
    a piece) and the literals the matcher left in the first one"""
    out, idx = oracle.compress_blocks(src, level, oracle.dfDeflate, FULL_BLOCK)
    assert out == oracle.compress(src, level, oracle.dfDeflate)
    types = [(int.from_bytes(out[b >> 3:(b >> 3) + 2], "little") >> (b & 7)) >> 1 & 3 for b, _ in idx[:-1]]
    return types, len(src) if level == 0 else oracle.block_tokens(src, level, 0, min(len(src), FULL_BLOCK))[3]


def huffman_depth(f):
    """depth of the unlimited Huffman tree of a histogram"""
    h = [(int(x), 0) for x in f if x]
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return h[0][1]


# ---- family C: crafted inputs for the hash-chain matcher (levels 2..9 and -1), each built to expose named mutants of
# tests/chain_model.py or to reach one structure of zh_chain_match.hip; what each reaches is asserted in
# tests/test_chain_craft.py from the model's statistics, the oracle's tokens and numpy ----
CHAIN_HASH_MUL = 0x1e35a7bd
CHAIN_HASH_INV = pow(CHAIN_HASH_MUL, -1, 1 << 32)
CHAIN_ALL_LEVELS = (2, 3, 4, 5, -1, 6, 7, 8, 9)
CHAIN_CONFIG = {2: (4, 16, 8), 3: (4, 32, 32), 4: (4, 16, 16), 5: (8, 32, 32), 6: (8, 128, 128), 7: (8, 256, 256),
                8: (32, 258, 1024), 9: (32, 258, 4096)}   # level: (good, nice, chain), internal.nim:177-189
CHAIN_DEVICE_LEVELS = (2, -1, 9)   # one level of wide link records, two of narrow ones
CHAIN_PERIODS = (1, 2, 3, 7, 129, 257, 258, 259)
CHAIN_GRID_AT = (0, 1, 32767, 32768, 32769, 65536)
CHAIN_GRID_DIST = (100, 32766, 32767, 32768, 32769)
CHAIN_BLOCK_SIZES = (32768, 65536)
CHAIN_TILE = 16384   # ZH_CHAIN_LINKS_TILE
chain_case_info = {}   # name -> what tests/test_chain_craft.py asserts of the case


def chain_hash(b, at=0):
    return ((int.from_bytes(b[at:at + 4], "little") * CHAIN_HASH_MUL) & 0xffffffff) >> 15


def chain_word(h, low15):
    """one of the 32 768 four-byte words of hash h"""
    return ((CHAIN_HASH_INV * ((h << 15) | low15)) & 0xffffffff).to_bytes(4, "little")


def chain_tag(b5):
    """zh_chain_tag of a position's first five bytes (zh_chain_match.hip), restated"""
    lo = int.from_bytes(b5[:4], "little")
    return ((lo * 0x9e3779b1 + b5[4] * 0x85ebca6b) & 0xffffffff) >> 16


def _c_decoy(h, avoid, rnd):
    """a word of hash h whose repeats hold no other position of hash h, and that shares no byte with `avoid`'s place"""
    while True:
        w = chain_word(h, rnd.randrange(32768))
        if w[0] != avoid[0] and all(chain_hash((w * 2)[k:k + 4]) != h for k in (1, 2, 3)):
            return w


def _c_levels(level):
    return (-1, 6) if level == 6 else (level,)


def _c_kills(level, *mutants):
    return {(lv, m) for lv in _c_levels(level) for m in mutants}


def _c_depth_cases(rnd):
    """depth: `n` words of the searcher's hash between a 20-byte target and its repeat; the target is candidate n + 1"""
    out = []
    for level, (good, nice, chain) in CHAIN_CONFIG.items():
        for n in (chain - 1, chain):
            h = rnd.randrange(1 << 17)
            x = chain_word(h, rnd.randrange(32768)) + rnd.randbytes(16)
            w = _c_decoy(h, x, rnd)
            pre = rnd.randbytes(37)
            src = pre + x + w * n + x + rnd.randbytes(9)
            found = n + 1 <= chain
            want = ["chain-1" if found else "chain+1"]
            for m, d in (("config-1", -1), ("config+1", 1)):
                other = CHAIN_CONFIG.get(level + d, (4, 8, 4) if level + d == 1 else None)
                if other is not None and (n + 1 <= other[2]) != found:
                    want.append(m)
            name = "C/depth/level%d_%d_decoys" % (level, n)
            chain_case_info[name] = dict(searcher=len(pre) + 20 + 4 * n, tried=chain, why=None if found else "tries",
                                         match=(len(pre) + 20 + 4 * n, 20 + 4 * n, 20) if found else None)
            out.append((name, src, _c_levels(level), _c_kills(level, *want)))
    return out


def _c_good_cases(rnd):
    """good: the nearest candidate matches good - 1 or good bytes; a 40-byte one is candidate 2 + ((chain - 1) >> 2),
    one more than a cut walk reaches and within what `tries >>= 1` would leave.  (good - 1 = 3 bytes at levels 2..4 is
    no candidate at all: words that share three bytes differ in the top byte, which the odd multiplier carries into the
    hash's top bits.)  cut: two candidates of `good` bytes, then 3 + (((chain - 1) >> 2) - 1 >> 2) deep the long one:
    the reference cuts once, `cut_always` twice.  At level 2 `cut_always` cannot show: after the first cut one try is
    left, ((8 - 1) >> 2) = 1, and the candidate that takes it is the last either way."""
    out = []
    for level, (good, nice, chain) in CHAIN_CONFIG.items():
        t1 = (chain - 1) >> 2
        for kind in ("good", "good-1", "cut"):
            if (kind == "good-1" and good - 1 < 4) or (kind == "cut" and level == 2):
                continue
            h = rnd.randrange(1 << 17)
            x = chain_word(h, rnd.randrange(32768)) + rnd.randbytes(36)
            w = _c_decoy(h, x, rnd)
            pre = rnd.randbytes(41)
            g = good - 1 if kind == "good-1" else good
            f1, f2 = x[:g] + bytes([x[g] ^ 0x55]), x[:g] + bytes([x[g] ^ 0xaa])
            if kind == "cut":
                body = w * ((t1 - 1) >> 2) + f2 + f1
                kills = _c_kills(level, "cut_always")
            else:
                body = w * t1 + f1
                kills = _c_kills(level, "good_gt", "shr1", *(("tag4",) if good == 4 else ())) if kind == "good" else set()
            src = pre + x + body + x + rnd.randbytes(9)
            at = len(pre) + 40 + len(body)
            name = "C/good/level%d_%s" % (level, kind)
            if kind == "good":
                chain_case_info[name] = dict(searcher=at, tried=1 + t1, why="tries", longest=g, cuts=1)
            else:
                chain_case_info[name] = dict(searcher=at, tried=t1 + 2 if kind == "good-1" else 3 + ((t1 - 1) >> 2),
                                             longest=40, cuts=1 if kind == "good-1" else 2, match=(at, len(body) + 40, 40))
            out.append((name, src, _c_levels(level), kills))
    return out


def _c_nice_cases(rnd):
    """nice: the nearest candidate matches nice - 1 or nice bytes, a longer one lies behind it.  Levels 8 and 9: nice
    is 258, the limit itself -- no candidate is longer than a 258-byte one, so `nice_gt` cannot show there; the
    257-byte case still tells level 8 from level 7 (`config-1`: nice 256 stops at 257 bytes)."""
    out = []
    for level, (good, nice, chain) in CHAIN_CONFIG.items():
        for m in (nice - 1, nice):
            if m == 258:
                continue
            h = rnd.randrange(1 << 17)
            x = chain_word(h, rnd.randrange(32768)) + rnd.randbytes(296)
            pre = rnd.randbytes(43)
            long_len = min(m + 20, 258)
            src = pre + x[:m + 20] + rnd.randbytes(5) + x[:m] + bytes([x[m] ^ 0x55]) + x[:m + 20] + rnd.randbytes(9)
            at = len(pre) + m + 20 + 5 + m + 1
            stops = m >= nice
            kills = _c_kills(level, "nice_gt") if stops else (_c_kills(level, "config-1") if level == 8 else set())
            name = "C/nice/level%d_%d_bytes" % (level, m)
            chain_case_info[name] = dict(searcher=at, tried=1 if stops else 2, why="nice" if stops else None,
                                         match=(at, m + 1, m) if stops else (at, at - len(pre), long_len))
            out.append((name, src, _c_levels(level), kills))
    return out


def _c_every_level_cases(rnd):
    """the decisions that no level's tuple touches: tie, min, sentinel, wrap, skip-insert, the block's last positions,
    the limit -- each input at every chain level"""
    out = []
    every = lambda *mutants: {(lv, m) for lv in CHAIN_ALL_LEVELS for m in mutants}

    def add(name, src, kills, **info):
        chain_case_info["C/" + name] = info
        out.append(("C/" + name, src, CHAIN_ALL_LEVELS, kills))
    # tie: two candidates of six bytes; the nearer one wins
    x = rnd.randbytes(6)
    src = rnd.randbytes(29) + x + b"\x01" + rnd.randbytes(10) + x + b"\x02" + rnd.randbytes(10) + x + b"\x03" + rnd.randbytes(9)
    add("tie/two_of_six_bytes", src, every("ge_longest"), match=(29 + 34, 17, 6))
    # min: longest matches of exactly 4, 5 and 6 bytes
    src, want = rnd.randbytes(31), []
    for n in (4, 5, 6):
        x = rnd.randbytes(n)
        src += x + b"\x01" + rnd.randbytes(12)
        if n > 4:
            want.append((len(src), n + 13, n))
        else:
            four_at = len(src)
        src += x + b"\x02" + rnd.randbytes(12)
    add("min/4_5_6_bytes", src, every("min4", "min6"), matches=want, searcher=four_at, longest=4)
    # skip-insert: a string that begins inside a hop (at its positions 1 and length - 1) is found there later
    a, e1, b, e2 = rnd.randbytes(30), rnd.randbytes(12), rnd.randbytes(30), rnd.randbytes(20)
    src = rnd.randbytes(33) + a + rnd.randbytes(9) + a + e1 + rnd.randbytes(9)
    want = [(len(src), 9 + 41, 41)]
    src += a[1:] + e1 + rnd.randbytes(9) + b + rnd.randbytes(9) + b + e2 + rnd.randbytes(9)
    want.append((len(src), 9 + 21, 21))
    src += b[29:] + e2 + rnd.randbytes(9)
    add("skip_insert/hop_positions_1_and_last", src, every("no_skip_insert"), matches_in=want, count=4)
    # the last positions: block_end - 5 is searched and finds its five bytes; block_end - 4 is not
    x = rnd.randbytes(5)
    src = rnd.randbytes(35) + x + rnd.randbytes(20) + x
    add("tail/five_bytes_at_end", src, every("min6"), match=(len(src) - 5, 25, 5))
    src = rnd.randbytes(35) + x + rnd.randbytes(20) + x[:4]
    add("tail/four_bytes_at_end", src, set(), matches=[])
    # limit: a repeat of 257, 258, 259 and 600 bytes
    for n in (257, 258, 259, 600):
        r = rnd.randbytes(n)
        src = rnd.randbytes(39) + r + rnd.randbytes(7) + r + rnd.randbytes(7)
        want = [(39 + n + 7 + k, n + 7, min(258, n - k)) for k in range(0, n, 258) if n - k > 4]
        add("limit/repeat_%d" % n, src, every("limit_259") if n > 258 else set(), matches=want)
    # ... and one that runs into the block's end (the search's 8-byte compare and its byte-by-byte tail)
    for k in (5, 8, 9, 257, 258):
        r = rnd.randbytes(300)
        src = rnd.randbytes(39) + r + rnd.randbytes(11) + r[:k]
        add("limit/%d_bytes_to_block_end" % k, src, set(), matches=[(350, 311, k)])
    # sentinel: a key in window slot 0 is never found; wrap: nor is one exactly a window back
    key = rnd.randbytes(20)
    add("sentinel/key_at_0_again_at_100", key + rnd.randbytes(80) + key + rnd.randbytes(10), every("no_sentinel"),
        matches=[(101, 100, 19)])   # (from the key's second byte on)
    key = rnd.randbytes(20)
    add("wrap/key_at_1_again_at_32769", b"\x00" + key + rnd.randbytes(32768 - 20) + key + rnd.randbytes(10), every("wrap_eq"),
        matches=[], searcher=32769, why="offset0")
    return out


def _c_grid_cases(rnd):
    """sentinel and wrap: a 20-byte key at block positions 0, 1, 32 767, 32 768, 32 769 and 65 536, again 100, 32 766,
    32 767, 32 768 and 32 769 bytes on, in noise.  Found: keys outside window slot 0 up to distance 32 767."""
    out = []
    for d in CHAIN_GRID_DIST:
        rest, part = list(CHAIN_GRID_AT), 0
        while rest:
            taken, spans = [], []
            for p in list(rest):
                mine = [(p, p + 20), (p + d, p + d + 20)]
                if all(hi <= lo2 or hi2 <= lo for lo, hi in mine for lo2, hi2 in spans):
                    taken.append(p)
                    spans += mine
                    rest.remove(p)
            src = bytearray(rnd.randbytes(max(taken) + d + 20 + 50))
            for p in taken:
                key = rnd.randbytes(20)
                src[p:p + 20] = key
                src[p + d:p + d + 20] = key
            name = "C/grid/distance_%d_part_%d" % (d, part)
            chain_case_info[name] = dict(grid=[(p, d, p % 32768 != 0 and d <= 32767) for p in taken])
            out.append((name, bytes(src), CHAIN_DEVICE_LEVELS, set()))
            part += 1
    return out


def _c_boundary(src, at, rnd):
    """around the block border `at`: a 40-byte string whose repeat starts 10 bytes in front of the border (clipped
    there), and a 30-byte string in the block's last bytes that comes again 50 bytes into the next block (not found)"""
    r, q = rnd.randbytes(40), rnd.randbytes(30)
    src[at - 2000:at - 1960] = r
    src[at - 10:at + 30] = r
    src[at - 40:at - 10] = q
    src[at + 50:at + 80] = q


def _c_block_cases(rnd):
    out = []
    src = bytearray(rnd.randbytes(65536 + 5000))
    _c_boundary(src, 32768, rnd)
    _c_boundary(src, 65536, rnd)
    kills = {(lv, m) for lv in CHAIN_ALL_LEVELS for m in ("head_survives_block", "limit_ignores_block_end")}
    chain_case_info["C/block/borders_32768_65536"] = dict(borders=(32768, 65536))
    out.append(("C/block/borders_32768_65536", bytes(src), CHAIN_ALL_LEVELS, kills))
    # two deflate blocks: most of the first is a run of one byte, which the parse crosses in 16 K hops
    src = bytearray(rnd.randbytes(3000) + b"\x6b" * (FULL_BLOCK - 6000) + rnd.randbytes(3000 + 70000))
    _c_boundary(src, FULL_BLOCK, rnd)
    chain_case_info["C/block/two_deflate_blocks"] = dict(borders=(FULL_BLOCK,), small=False)
    out.append(("C/block/two_deflate_blocks", bytes(src), (2, 9), set()))
    return out


def _c_tiny_cases():
    out = []
    for n in range(5, 14):
        out.append(("C/tiny/one_byte_%d" % n, b"\xc4" * n, CHAIN_ALL_LEVELS, set()))
        out.append(("C/tiny/distinct_%d" % n, bytes(range(65, 65 + n)), CHAIN_ALL_LEVELS, set()))
        # (position 1's candidate is window slot 0, the sentinel; position 2 finds position 1 from 7 bytes on)
        chain_case_info["C/tiny/one_byte_%d" % n] = dict(matches=[(2, 1, n - 2)] if n >= 7 else [])
        chain_case_info["C/tiny/distinct_%d" % n] = dict(matches=[])
    return out


def _c_tag_case(rnd):
    """tags: five-byte strings of the searcher's hash AND the searcher's zh_chain_tag whose bytes differ, as candidates
    in front of a true 20-byte match: the narrow records say "may match", the bytes say no"""
    h = rnd.randrange(1 << 17)
    words = (np.uint32(CHAIN_HASH_INV) * ((np.uint32(h) << np.uint32(15)) | np.arange(32768, dtype=np.uint32)))
    tags = (words * np.uint32(0x9e3779b1))[:, None] + np.arange(256, dtype=np.uint32)[None, :] * np.uint32(0x85ebca6b) >> np.uint32(16)
    mine = int(tags[0, 0x41])
    hits = [(int(i), int(b)) for i, b in np.argwhere(tags == mine) if i != 0][:5]
    assert len(hits) == 5
    s5 = int(words[0]).to_bytes(4, "little") + b"\x41"
    cands = [int(words[i]).to_bytes(4, "little") + bytes([b]) for i, b in hits]
    x = s5 + rnd.randbytes(15)
    pre = rnd.randbytes(45)
    body = b"".join(c + rnd.randbytes(2) for c in cands)
    src = pre + x + rnd.randbytes(3) + body + x + rnd.randbytes(9)
    at = len(pre) + 23 + len(body)
    chain_case_info["C/tags/equal_tag_other_bytes"] = dict(searcher=at, tried=6, match=(at, 23 + len(body), 20), searcher5=s5,
                                                          candidates=cands)
    return [("C/tags/equal_tag_other_bytes", src, (2, 5, -1, 9), set())]


def chain_classes(src):
    """the class (low five bits of the hash) of every inserted position of a one-block input"""
    a = np.frombuffer(src, np.uint8).astype(np.uint32)
    n = len(src) - 4
    w = a[:n] | a[1:n + 1] << 8 | a[2:n + 2] << 16 | a[3:n + 3] << 24
    return ((w * np.uint32(CHAIN_HASH_MUL)) >> np.uint32(15)) & np.uint32(31)


def _c_class_case(rnd):
    """classes and tiles: 3 tiles + 100 positions; the first tile is a run (one class holds all of it), the second
    and third noise over two letters (<= 16 classes), and in the third a stretch of a third letter brings a class
    that no earlier position has; <= 23 classes in all, so some stay empty"""
    total = 3 * CHAIN_TILE + 100
    for _ in range(1000):
        a, b, c = rnd.sample(range(256), 3)
        two = lambda n: bytes(rnd.choice((a, b)) for _ in range(n))
        third = two(8000) + bytes([a] * 4 + [c] * 8 + [a] * 4)
        src = bytes([a]) * CHAIN_TILE + bytes([a] * 3) + two(CHAIN_TILE - 3) + third
        src += two(total + 4 - len(src))
        cls = chain_classes(src)
        early = set(cls[:2 * CHAIN_TILE].tolist())
        if len(set(cls[:CHAIN_TILE].tolist())) == 1 and set(cls[2 * CHAIN_TILE:].tolist()) - early:
            return [("C/classes/three_tiles", src, CHAIN_DEVICE_LEVELS, set())]
    raise AssertionError("no letters found")


def _c_device_cases(rnd):
    out = []

    def add(name, src, keep=True, **info):
        chain_case_info["C/" + name] = dict(info, small=keep)
        out.append(("C/" + name, src, CHAIN_DEVICE_LEVELS, set()))
    # never-meeting walks: back-to-back 258-byte matches over three fragments and a bit
    for p in CHAIN_PERIODS:
        unit = bytes(rnd.sample(range(256), min(p, 256))) + rnd.randbytes(max(0, p - 256))
        add("runs/period_%d" % p, (unit * (3 * FRAG // p + 1000))[:3 * FRAG + 1000], p in (1, 258), period=p)
    # spill: matches that end at a fragment's border and 1, 2, 257 bytes behind it, or start 1 and 5 bytes in front
    for start, n in ((FRAG - 100, 100), (FRAG - 99, 100), (FRAG - 98, 100), (FRAG - 1, 258), (FRAG - 5, 100)):
        src = bytearray(rnd.randbytes(FRAG + 1500))
        src[start:start + n] = src[1000:1000 + n]
        add("spill/match_%d_of_%d" % (start, n), bytes(src), (start, n) in ((FRAG - 100, 100), (FRAG - 1, 258)),
            matches_at=(start, start - 1000, n))
    # crowded fragment: 5459 five-byte words, each behind a separator that ends the match
    words = set()
    while len(words) < 5459:
        words.add(rnd.randbytes(5))
    words = sorted(words)
    rnd.shuffle(words)
    first = b"".join(w + bytes([1 + i % 100]) for i, w in enumerate(words))
    second = b"".join(w + bytes([101 + i % 100]) for i, w in enumerate(words))
    add("crowded/fragment_of_5459_matches", rnd.randbytes(8) + first + rnd.randbytes(FRAG - 8 - len(first)) + second + b"\xee\xee")
    return out


_chain_craft_cache = {}


def chain_crafted_inputs(small=False):
    """Family C -> [(name, bytes, levels, kills)]; kills: the (level, mutant) pairs of tests/chain_model.py that the
    input is built to tell from the reference.  small: the emulator's subset -- every cell, at levels 2, -1 and 9 only,
    without the two-block input."""
    if False not in _chain_craft_cache:
        rnd = random.Random(2718)
        cases = (_c_depth_cases(rnd) + _c_good_cases(rnd) + _c_nice_cases(rnd) + _c_every_level_cases(rnd) + _c_grid_cases(rnd) +
                 _c_block_cases(rnd) + _c_tiny_cases() + _c_tag_case(rnd) + _c_class_case(rnd) + _c_device_cases(rnd))
        assert len({c[0] for c in cases}) == len(cases)
        _chain_craft_cache[False] = cases
        keep = []
        for name, src, levels, kills in cases:
            levels = tuple(lv for lv in levels if lv in CHAIN_DEVICE_LEVELS)
            if levels and chain_case_info.get(name, {}).get("small", True) and \
                    (name.split("/")[1] != "grid" or name.endswith("part_0")) and \
                    (name.split("/")[1] != "tiny" or name.endswith(("_5", "_7", "_8", "_13"))):
                keep.append((name, src, levels, {k for k in kills if k[0] in levels}))
        _chain_craft_cache[True] = keep
    return list(_chain_craft_cache[small])


def chain_block_cases(small=False):
    """the cases of family C that go through the block-parallel form (check_blocks) as well"""
    return [c for c in chain_crafted_inputs(small) if c[0] == "C/block/borders_32768_65536"]


def check_chain_crafted(eng, small=False, levels=None):
    """family C on a device: the oracle's bytes (gzip, one batch a level), then the oracle's tokens case by case"""
    cases = chain_crafted_inputs(small)
    if levels is not None:
        cases = [(n, s, tuple(lv for lv in own if lv in levels), k) for n, s, own, k in cases]
    check_crafted_compress(eng, [(n, s, own, GZIP_ONLY) for n, s, own, _ in cases])
    for name, src, own, _ in cases:
        for level in own:
            try:
                check_tokens(eng, src, level)
            except AssertionError as e:
                raise AssertionError("%s: %s" % (name, e))


# ---- family P: crafted inputs for the parallel BestSpeed parse (contract mode, zh_l1p_match.hip), each built to expose
# named mutants of tests/l1p_model.py or to reach one thing the kernel's speculation has to get right; what each reaches
# is asserted in tests/test_l1p_craft.py from the model alone ----
L1P_CHUNK = 32      # positions a parse thread of the kernel
L1P_WAVE = 2048     # positions a wave of parse threads
L1P_TAIL_LENGTHS = (15, 16, 17, 19, 20, 63, 64, 65, 32767, 32768, 32768 + 15, 32768 + 16, 32768 + 19)
L1P_BACK_TO_BACK = (31, 32, 33)
L1P_PERIODS = (1, 31, 33, 258, 259)
L1P_DENSE_WORDS = 97   # a prime: every ordered pair of different words once (97 * 96 * 4 bytes > a fragment)
L1P_ALIGN_TEXT = "P/text/40001"
l1p_case_info = {}   # name -> what tests/test_l1p_craft.py asserts of the case


def l1p_hash(b, at=0):
    return (int.from_bytes(b[at:at + 4], "little") * CHAIN_HASH_MUL) & 0xffffffff


def every_pair_once(k):
    """0 .. k-1 (k prime) in an order where every ordered pair of different neighbours comes exactly once: for each
    step d the cycle 0, d, 2d, ... back to 0"""
    seq = [0]
    for d in range(1, k):
        seq += [j * d % k for j in range(1, k + 1)]
    return seq


def _p_units(rnd, k, size):
    """k strings of `size` bytes with pairwise different first bytes and pairwise different slots of their first words"""
    units, slots = [], set()
    while len(units) < k:
        u = bytes([32 + len(units)]) + rnd.randbytes(size - 1)
        if l1p_hash(u) >> 18 not in slots:
            slots.add(l1p_hash(u) >> 18)
            units.append(u)
    return units


def _p_two_frags(rnd):
    """the word at 300 in fragment 0 and at 100 and 400 in fragment 1; fragment 0 is a byte ramp behind 400 (few
    words, few slots), and the word is drawn until no later position of fragment 0 takes its slot"""
    import l1p_model as lm
    ramp = bytes(range(256)) * (FRAG // 256)
    f0 = rnd.randbytes(300)
    f1 = rnd.randbytes(600)
    for _ in range(64):
        key = rnd.randbytes(16)
        src = f0 + key + ramp[316:] + f1[:100] + key + f1[116:400] + key + f1[416:]
        if lm.model(src, "table_survives") != lm.model(src):
            return src
    raise AssertionError("no word found")


def l1p_crafted_inputs():
    """Family P -> [(name, bytes, kills)]; kills: the mutants of tests/l1p_model.py that the input is built to tell from
    the rule.  At most three fragments each."""
    if "P" in _compress_craft_cache:
        return list(_compress_craft_cache["P"])
    rnd = random.Random(1618)
    alice = synth.corpus_file("alice29.txt")
    html = synth.corpus_file("html")
    out = []
    info = l1p_case_info

    def add(name, src, kills=(), **claims):
        out.append(("P/" + name, bytes(src), frozenset(kills)))
        info["P/" + name] = claims

    # -- the last 15 bytes: a repeat that starts exactly 16, and one exactly 15, bytes before the end
    key = rnd.randbytes(16)
    body = rnd.randbytes(484)
    add("tail/repeat_at_n-16", body[:100] + key + body[100:] + key, {"tail17"}, has=[(500, 400, 16)])
    add("tail/repeat_at_n-15", body[:100] + key[:15] + body[100:] + key[:15], {"tail15"}, none_from=499)
    # -- the cap: a 300-byte repeat
    key = rnd.randbytes(300)
    add("cap/repeat_300", body[:50] + key + body[50:100] + key + body[100:200], {"lim257", "lim259"},
        has=[(400, 350, 258)])
    add("cap/run_300", body[:50] + b"\x5a" * 300 + body[50:150], {"lim257", "lim259"}, has=[(51, 1, 258), (309, 1, 41)])
    # -- a repeat cut by the fragment's end whose continuation matches in the next fragment
    key = rnd.randbytes(200)
    noise = rnd.randbytes(FRAG + 500)
    add("frag/repeat_cut_at_32768", noise[:FRAG - 400] + key + noise[FRAG - 200:FRAG - 100] + key + noise[FRAG + 100:],
        {"lim_past_frag"}, has=[(FRAG - 100, 300, 100)])
    # -- position 0 is no candidate
    key = rnd.randbytes(16)
    add("pos0/only_occurrence_at_0", key + body[:100] + key + body[100:150], {"pos0"}, has=[(117, 116, 15)], none_at=[116])
    # -- the minimum: a four-byte repeat
    add("min/four_byte_repeat", body[:40] + b"WXYZ" + body[40:90] + b"WXYZ" + body[90:140], {"min5"}, has=[(94, 54, 4)])
    # -- a candidate inside a taken match: every position enters the table
    key = rnd.randbytes(30)
    add("table/candidate_inside_a_match", body[:10] + key + body[10:20] + key + body[20:60] + key[5:25] + body[60:100],
        {"visited_only"}, has=[(50, 40, 30), (120, 65, 20)])
    # -- a word, its repeat and a third copy inside one 64-position step: the earlier one is the candidate, never the later
    key = rnd.randbytes(8)
    add("same-step/three_in_64_127", body[:70] + key + body[70:82] + key + body[82:94] + key + body[94:250],
        {"step_granular"}, has=[(90, 20, 8), (110, 20, 8)])
    add("two-frags/table_of_fragment_0", _p_two_frags(rnd), {"table_survives"}, has=[(FRAG + 400, 300, 16)])
    # -- fragment lengths: text, the last 8 + k bytes one letter (so that a last fragment of k bytes has something to find)
    for n in L1P_TAIL_LENGTHS:
        k = n % FRAG or FRAG
        src = (alice[3000:3000 + n - k] + b"q" * k) if k <= 65 else alice[3000:3000 + n - 40] + b"q" * 40
        add("len/%d" % n, src, has=[(n - k + 2, 1, k - 2)] if 19 <= k <= 65 else [], none_from=n - k if k < 18 else n - 15)
    # -- zeros up to and across a fragment's end (the kernel's compare runs into zeroed slack behind the fragment)
    add("zeros/up_to_fragment_end", noise[:FRAG - 1000] + bytes(1000) + noise[FRAG:], ends_at=[FRAG])
    add("zeros/across_fragment_end", noise[:FRAG - 500] + bytes(1000) + noise[FRAG:FRAG + 300], {"lim_past_frag"},
        ends_at=[FRAG], has=[(FRAG + 2, 1, 258)])
    add("zeros/two_fragments_and_19", bytes(2 * FRAG + 19), ends_at=[FRAG, 2 * FRAG, 2 * FRAG + 19])
    # -- periods: matches of 258 back to back, whose phase against the kernel's chunks drifts
    for p in L1P_PERIODS:
        add("period/%d" % p, (rnd.randbytes(p) * (2200 // p + 2))[:2200], period=p)
    add("period/258_two_fragments", (rnd.randbytes(258) * 200)[:FRAG + 1000], period=258)
    add("period/259_two_fragments", (rnd.randbytes(259) * 200)[:FRAG + 1000], period=259)
    # -- matches of 31, 32, 33 bytes back to back through a whole fragment: 37 strings in an order where no pair of
    # neighbours repeats, so every match ends where its string ends
    for size in L1P_BACK_TO_BACK:
        units = _p_units(rnd, 37, size)
        add("spec/back_to_back_%d" % size, b"".join(units[i] for i in every_pair_once(37))[:FRAG], back_to_back=size)
    # -- a match that ends exactly on a chunk edge, and one on a wave edge
    key = rnd.randbytes(40)
    add("spec/ends_on_chunk_edge", body[:5] + key[:20] + body[5:56] + key[:20] + body[56:250], has=[(76, 71, 20)])
    add("spec/ends_on_wave_edge", noise[:1900] + key + noise[1940:2008] + key + noise[2048:2300], has=[(2008, 108, 40)])
    # -- a phase pair: period 33 through a whole fragment; the second input's periodicity begins 6 bytes earlier
    pattern = rnd.randbytes(33)
    head = rnd.randbytes(19) + bytes([pattern[-1] ^ 0x55])
    add("spec/phase_a", head + (pattern * 1000)[:FRAG - 20])
    add("spec/phase_b", head[:14] + pattern[-6:] + (pattern * 1000)[:FRAG - 20])
    # -- text: walks from different entries meet (a thread that walks its chunk again knows some lengths already)
    add("text/one_fragment", alice[20000:20000 + FRAG])
    add("text/40001", html[5000:45001])
    add("text/three_fragments", alice[:40000] + html[:2 * FRAG + 19 - 40000])
    # -- dense: a four-byte match every four bytes, close to the fragment's room for match records
    units = _p_units(rnd, L1P_DENSE_WORDS, 4)
    add("dense/four_byte_matches", b"".join(units[i] for i in every_pair_once(L1P_DENSE_WORDS))[:FRAG], {"min5"})
    assert len({c[0] for c in out}) == len(out) and all(len(c[1]) <= 3 * FRAG for c in out)
    _compress_craft_cache["P"] = out
    return list(out)


_l1p_model_cache = {}


def l1p_model_of(name, src):
    """tests/l1p_model.py's matches of a named input, worked out once a process"""
    import l1p_model as lm
    if name not in _l1p_model_cache:
        _l1p_model_cache[name] = (src, lm.model(src))
    assert _l1p_model_cache[name][0] == src, name
    return _l1p_model_cache[name][1]


def l1p_token_cases(small=False):
    """what check_l1p_tokens runs: family P, edge_inputs(), two `synth` mix buffers of 70000 bytes and family M
    (small: M's subset for the emulator) -> [(name, bytes)]"""
    cases = [(n, s) for n, s, _ in l1p_crafted_inputs()]
    cases += [("edge/%d" % i, s) for i, s in enumerate(edge_inputs())]
    cases += [("mix/%d" % i, b.tobytes()) for i, b in enumerate(synth.gen_batch("mix", 2, 70000, first_index=40))]
    cases += [(c[0], c[1]) for c in crafted_inputs(small) if c[0].startswith("M/")]
    return cases


def l1p_same_step_cases(cases):
    """the names of the cases whose tokens, by the model, depend on a candidate that entered the table in the same
    64-position step as its position (a device that serves a step's lanes in another order may not see it)"""
    import l1p_model as lm
    return {name for name, src in cases if lm.model(src, "step_granular") != l1p_model_of(name, src)}


def check_l1p_tokens(eng, cases, skip=()):
    """Contract mode's tokens (zh_debug_tokens follows the switch) are the rule's, token for token: the matches of
    tests/l1p_model.py in order, covering the input.  skip: names left out, each printed with its reason."""
    bad = []
    eng.set_l1_parse(1)
    try:
        for name, src in cases:
            if name in skip:
                print("check_l1p_tokens: %s left out: its tokens depend on a same-step candidate, and this device does "
                      "not serve a step's lanes in ascending order" % name)
                continue
            got, covered = token_matches(eng.debug_tokens(src, 1))
            want = l1p_model_of(name, src)
            if got != want or covered != len(src):
                k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
                bad.append((name, "token %d" % k, "device", got[k:k + 2], "model", want[k:k + 2], "covered", covered, len(src)))
    finally:
        eng.set_l1_parse(-1)
    assert not bad, bad


def l1p_multi_fragment_cases():
    """the cases one workgroup has to take fragment after fragment under ZH_L1P_SLOTS=1: family P's inputs of more than
    one fragment"""
    return [(n, s) for n, s, _ in l1p_crafted_inputs() if len(s) > FRAG]


def check_l1p_one_slot(preamble, skip=()):
    """check_l1p_tokens over l1p_multi_fragment_cases() in a child process with ZH_L1P_SLOTS=1 (read once a process):
    one persistent workgroup takes every fragment of a buffer.  preamble: Python source that leaves the engine in `eng`;
    skip: as check_l1p_tokens takes it."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" % (here, os.path.dirname(here)) + preamble +
            "\nimport parity_cases as pc\n"
            "pc.check_l1p_tokens(eng, pc.l1p_multi_fragment_cases(), %r)\n" % (tuple(sorted(skip)),))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ZH_L1P_SLOTS="1"), capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])


def check_l1p_alignment(eng, upload, download, alloc):
    """One family P text at source offsets of all four alignments modulo 4, level 1 in contract mode: in one
    compress_batch with 1-, 2- and 3-byte buffers between the copies, and through the device plan API at unaligned
    offsets -- every copy gives the bytes the buffer gives alone, and its tokens are the model's.  (The host batch
    stages every source in a slot of its own, aligned: it is the device plan that moves the fragments off the dwords.
    A full fragment there once lost its last 1..3 bytes to the zeroed slack: streams that did not decode.)"""
    name, text = next((n, s) for n, s, _ in l1p_crafted_inputs() if n == L1P_ALIGN_TEXT)
    assert len(text) == 40001
    eng.set_gzip_fname_len(0)
    eng.set_l1_parse(1)
    try:
        alone = eng.compress(text, 1, oracle.dfDeflate)
        assert zlib.decompress(alone, -15) == text
        batch = [text, b"a", text, b"bc", text, b"def", text]
        outs, sts = eng.compress_batch(batch, 1, oracle.dfDeflate)
        assert all(st == 0 for st in sts)
        assert [outs[i] == alone for i in (0, 2, 4, 6)] == [True] * 4, "the stream depends on the source's alignment"
        blob, soff = bytearray(), []
        for want, pad in zip((3, 2, 1, 0), (3, 1, 7, 2)):   # at least `pad` bytes of something else in front, then up to `want`
            blob += b"\xaa" * pad
            blob += b"\xaa" * ((want - len(blob)) % 4)
            soff.append(len(blob))
            blob += text
        assert [o % 4 for o in soff] == [3, 2, 1, 0]
        d_src, keep_src = upload(bytes(blob) + b"\0" * 64)
        cap = eng.compress_bound(len(text))
        doff = [5 + i * (cap + 3) for i in range(4)]
        d_dst, keep_dst = alloc(doff[-1] + cap + 64, 0xAB)
        plan = eng.plan_compress(soff, [len(text)] * 4, doff, [cap] * 4, 1, oracle.dfDeflate)
        plan.run(d_src, d_dst)
        lens, sts = plan.results()
        assert list(sts) == [0] * 4
        host = download(keep_dst)
        for o, n in zip(doff, lens):
            assert host[o:o + n] == alone, "device API: the stream depends on the source's alignment (offset %d)" % o
    finally:
        eng.set_l1_parse(-1)
    assert _stream_matches(dc.read_blocks(alone)) == l1p_model_of(name, text)


def _stream_matches(blocks):
    """read_blocks' tokens -> [(position, offset, length)]"""
    out, pos = [], 0
    for blk in blocks:
        for t in blk["tokens"]:
            if t[0] == "lit":
                pos += 1
            else:
                out.append((pos, t[2], t[1]))
                pos += t[1]
    return out


def check_l1p_streams(eng):
    """Family P compressed to dfDeflate in contract mode, read back with deflate_craft.read_blocks: the stream's
    matches are the model's and its tokens cover the input (the literal runs need not be cut alike); in every dynamic
    block the header's code lengths are those zh_debug_huffman(contract) makes of the histogram counted from that
    block's own tokens plus the end-of-block symbol, for both alphabets -- so the fragment histograms the matcher wrote
    are exact.  -> the number of dynamic blocks that hold matches."""
    cases = l1p_crafted_inputs()
    eng.set_l1_parse(1)
    try:
        outs, sts = eng.compress_batch([c[1] for c in cases], 1, oracle.dfDeflate)
    finally:
        eng.set_l1_parse(-1)
    dynamic_with_matches = 0
    for (name, src, _), out, st in zip(cases, outs, sts):
        assert st == 0, (name, st)
        blocks = dc.read_blocks(out)
        assert dc.replay(blocks) == src, name
        if {blk["type"] for blk in blocks} == {0}:   # (noise around one repeat: the block is stored, its matches dropped)
            continue
        assert _stream_matches(blocks) == l1p_model_of(name, src), name
        for k, blk in enumerate(blocks):
            if blk["type"] != 2:
                continue
            lit, dist = np.zeros(286, np.uint32), np.zeros(30, np.uint32)
            lit[256] = 1
            for t in blk["tokens"]:
                if t[0] == "lit":
                    lit[t[1]] += 1
                else:
                    lit[257 + (28 if t[1] == 258 else max(i for i in range(28) if dc.LEN_BASE[i] <= t[1]))] += 1
                    dist[max(i for i in range(30) if dc.DIST_BASE[i] <= t[2])] += 1
            _, lit_lens = eng.debug_huffman(lit, 257, 15, contract=True)
            _, dist_lens = eng.debug_huffman(dist, 2, 15, contract=True)
            assert list(lit_lens[:len(blk["lit_lens"])]) == blk["lit_lens"] and not any(lit_lens[len(blk["lit_lens"]):]), (name, k, "litlen")
            assert list(dist_lens[:len(blk["dist_lens"])]) == blk["dist_lens"] and not any(dist_lens[len(blk["dist_lens"]):]), (name, k, "distance")
            dynamic_with_matches += bool(dist.any())
    assert dynamic_with_matches >= 1
    return dynamic_with_matches
