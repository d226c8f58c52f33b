"""CPU checks of tests/zip_v1_reader_model.py, the restatement of ZipArchive.open (ziparchives_v1.nim:105-329) that the
device tests of zh_zip_read_batch compare against: archives of Python's zipfile and of the v1 writer's model open to
their inputs, the reference's own fixtures and the v2 writer's archives are refused where the reference refuses them,
and the cases of tests/zip_read_cases.py have the statuses they were built for."""
import io
import zipfile

import pytest

import zip_read_cases as zc
import zip_v1_reader_model as zm
import zip_v1_writer_model as wm
from oracle import zip_oracle

MEMBERS = [("dir/", b""), ("dir/a.txt", b"alpha" * 40), ("dir/b.bin", zc.blob(3000)), ("empty", b"")]


@pytest.mark.parametrize("compression", [zipfile.ZIP_STORED, zipfile.ZIP_DEFLATED])
def test_model_opens_zipfile_images(compression):
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", compression) as zf:
        for name, data in MEMBERS:
            zf.writestr(zipfile.ZipInfo(name, (2020, 1, 2, 3, 4, 6)), data, compression)
    st, table, _ = zm.expected(buf.getvalue())
    assert st == 0
    assert [(k.decode(), v["contents"]) for k, v in table.items()] == MEMBERS
    date, time = (2020 - 1980) << 9 | 1 << 5 | 2, 3 << 11 | 4 << 5 | 3
    assert all((v["dos_time"], v["dos_date"], v["in_directory"]) == (time, date, 1) for v in table.values())


def test_model_on_the_reference_fixtures():
    bagnon = zc.fixture("Bagnon-10.2.31.zip")
    assert bagnon[6] & 8 and zm.expected(bagnon)[0] == zc.DEFLATE64  # flag bit 3 of record 0
    assert zm.expected(zc.fixture("cat.jpg"))[0] == zc.OPEN


@pytest.mark.parametrize("level", [-2, 0, 1, -1, 9])
def test_model_opens_the_v1_writer_models_archives(level):
    entries = [("d/", (b"", True, 0x6000, 0x5521)), ("e", b""), ("h.txt", (b"Hello, World!", False, 7, 9)),
               ("big.bin", zc.blob(40000, 3)), (".hidden", b"stored by its name")]
    st, table, _ = zm.expected(wm.image(entries, level))
    assert st == 0
    want = wm.normalize(entries)
    assert [(k.decode(), v["contents"], v["is_directory"], v["dos_time"], v["dos_date"]) for k, v in table.items()] == [
        (p if isinstance(p, str) else p.decode(), c, d, t, dd) for p, c, d, t, dd in want]
    assert all(v["in_directory"] == 1 for v in table.values())


def test_model_refuses_the_v2_writers_archives():
    """createZipArchive writes ff ff ff ff sizes into its local headers: the data lie beyond the image"""
    image = zip_oracle.create_archive([("k/x.txt", b"x" * 999), ("k/y.txt", zc.blob(2500, 5)), ("k/z", b"")])
    assert zm.expected(image)[0] == zc.ARCHIVE_EOF


ALL = zc.scan_geometry() + zc.straddling_pair() + zc.chains() + zc.decoys() + zc.statuses() + zc.tables()


@pytest.mark.parametrize("name,image,status", ALL, ids=[x[0] for x in ALL])
def test_cases_have_the_status_they_were_built_for(name, image, status):
    st, table, stop = zm.expected(image)
    assert (zc.DECODER if st is None else st) == status
    assert (table is not None) == (status == zc.OK)


def test_case_tables():
    cases = {x[0]: zm.expected(x[1])[1] for x in zc.tables() + zc.decoys()}
    t = cases["duplicate_key"]
    assert list(t) == [b"a", b"b", b"c"] and t[b"a"]["contents"] == b"second, and longer"
    assert (t[b"a"]["dos_time"], t[b"a"]["dos_date"], t[b"a"]["in_directory"]) == (3, 4, 0)
    assert list(cases["backslash_and_slash"]) == [b"a/b", b"c"] and cases["backslash_and_slash"][b"a/b"]["contents"] == b"2"
    t = cases["two_centrals"]
    assert t[b"b"]["is_directory"] and t[b"b"]["unix_mode"] == 0o100600 and t[b"c"]["unix_mode"] == 0
    assert [v["in_directory"] for v in cases["some_central_records"].values()] == [0, 1]
    assert cases["directory_with_bytes"][b"d/"]["contents"] == b"kept"
    for name, _, _ in zc.decoys():
        assert not any(b"decoy" in k for k in cases[name]) or name == "in_name", name


def test_mixed_generator_is_mixed():
    """the 256 mixed archives by the model alone: more than half open and at least 6 distinct statuses occur, so the
    batch tests cannot pass on failures alone"""
    sts = [zm.expected(image)[0] for image in zc.random_images(20261018, 256)]
    opened = sum(1 for s in sts if s == 0)
    assert opened > 128 and len(set(sts)) >= 6, (opened, set(sts))
