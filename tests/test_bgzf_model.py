"""CPU-only: tests/bgzf_model.py (BGZF restated in plain Python) held against Python's own gzip and against the
statuses the cases of tests/bgzf_cases.py were built for.  No engine: the decoder is the oracle's."""
import gzip

import pytest

import bgzf_cases as bc
import bgzf_model as bm
import oracle


def test_model_written_files_read_back_through_gzip():
    for b in (7, 4096, 65280):
        for i, n in enumerate(bc.lengths(b)):
            src = bc.pattern(n, 1 + i)
            for level in (-2, 0, 6):
                image = bc.written(src, level, b)
                assert gzip.decompress(image) == src
                assert bm.read(image) == (bm.OK, src, 1)
                st, idx, eof = bm.index(image)
                assert (st, eof) == (bm.OK, 1) and len(idx) == (n + b - 1) // b + 2
                assert idx[-1] == (len(image), n) and idx[-2][0] == len(image) - 28


def test_model_empty_source_is_the_marker_alone():
    assert bm.write(b"", 1) == bm.EOF == bm.member(b"\x03\x00", 0, 0)
    assert gzip.decompress(bm.EOF) == b""
    assert bm.read(b"") == (bm.OK, b"", 0) and bm.index(b"") == (bm.OK, [(0, 0)], 0)


def test_model_fallback_lies_on_both_sides_of_a_member():
    big, small = bc.fallback_pair()
    nbig = len(oracle.compress(big, -2, oracle.dfDeflate))
    nsmall = len(oracle.compress(small, -2, oracle.dfDeflate))
    print("level -2: %d random bytes -> %d, %d -> %d" % (len(big), nbig, len(small), nsmall))
    assert nsmall <= bm.MAX_CDATA < nbig
    assert len(bm.cdata_of(big, -2)) == 5 + len(big) and len(bm.cdata_of(small, -2)) == nsmall
    for src in (big, small):
        assert gzip.decompress(bm.write(src, -2, 65505)) == src


def test_model_good_images():
    for name, image, data in bc.good_images():
        assert gzip.decompress(image) == data, name
        st, got, eof = bm.read(image)
        assert (st, got) == (bm.OK, data), name
        assert eof == (1 if image.endswith(bm.EOF) else 0), name
    image, src = bc.many_members()
    assert gzip.decompress(image) == src and len(bm.index(image)[1]) == 1602


@pytest.mark.parametrize("case", bc.bad_images(), ids=lambda c: c[0])
def test_model_bad_images_have_the_status_they_were_built_for(case):
    name, image, want = case
    st, data, eof = bm.read(image)
    assert data is None and eof == 0 or want in (bm.SIZE, bm.CHECKSUM, None)
    if want is None:
        assert st not in (bm.OK, bm.SIZE, bm.CHECKSUM, bm.BGZF_HEADER)  # a status of the decoder's own
    else:
        assert st == want


def test_model_signature_across_images():
    images, want = bc.straddling_pair()
    assert [bm.read(x)[0] for x in images] == want
    assert images[0].endswith(b"\x1f\x8b\x08") and images[1][:1] == b"\x04" and len(images[0]) % 8 == 0


def test_model_ranges_are_slices():
    srcs, images = bc.range_files(2)
    idx = [bm.index(x)[1] for x in images]
    rr = [(0, 0, 1), (0, bc.RB - 3, 10), (1, 5, 5 * bc.RB), (0, len(srcs[0]) - 1, 9), (0, len(srcs[0]), 9), (1, 7, 0)]
    outs, sts = bm.ranges(images, idx, rr)
    assert sts == [0] * len(rr) and outs == [srcs[t][o:o + n] for t, o, n in rr]
    assert bm.ranges(images, [idx[0], idx[1][:3] + [(0, 0)]], [(1, 0, 1), (0, 0, 1)])[1] == [bm.INVALID_BUFFER, 0]
