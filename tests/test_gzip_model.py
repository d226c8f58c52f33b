"""CPU-only: tests/gzip_model.py, the model zh_gzip_read_batch is held against, is itself held against Python's gzip on
every sound image of tests/gzip_cases.py, and its header checks and verdict order against hand-made faults.  No engine:
a stream zlib refuses gets a status of this file's choosing."""
import gzip
import struct
import zlib

import pytest

import gzip_cases as gc
import gzip_model as gm

REFUSED = 13


def refuse(src):
    return REFUSED


def sound_images():
    images = [b"".join(gc.members(k, seed=k)) for k in (0, 1, 2, 3, 64, 65)]
    images += [gc.member(plain, raw=raw) + gc.member(b"tail") for _, _, raw, plain in gc.crafted_streams()]
    images += gc.straddling_images()[0][:32]
    images += [b for b in gc.fixtures(256 * 1024) if gm.read(b, refuse)[0] == gm.OK]
    images.append(images[1] + b"\0" * 511)
    return images


def test_model_equals_python_gzip_on_sound_images():
    images = sound_images()
    assert len(images) > 60
    for im in images:
        st, data, recs = gm.read(im, refuse)
        assert st == gm.OK
        assert data == gzip.decompress(im)
        assert sum(r["ulen"] for r in recs) == len(data)
        for r in recs:
            body = im[r["cdata_off"]:r["cdata_off"] + r["cdata_len"]]
            assert zlib.decompress(body, -15) == data[r["uoff"]:r["uoff"] + r["ulen"]]
            assert (r["crc"], r["isize"]) == struct.unpack_from("<II", im, r["cdata_off"] + r["cdata_len"])


def test_model_reads_the_fields():
    m = gc.member(b"data", extra=b"\x01\x02\x03", name=b"name", comment=b"words", hcrc=True, mtime=77, xfl=2, os_=3, ftext=True)
    st, data, (r,) = gm.read(m, refuse)
    assert st == gm.OK and data == b"data"
    assert (r["flg"], r["mtime"], r["xfl"], r["os"]) == (31, 77, 2, 3)
    assert (r["extra_off"], r["extra_len"]) == (12, 3)
    assert m[r["name_off"]:r["name_off"] + r["name_len"]] == b"name"
    assert m[r["comment_off"]:r["comment_off"] + r["comment_len"]] == b"words"
    assert r["cdata_off"] == r["comment_off"] + 5 + 1 + 2 and r["coff"] == 0 and r["uoff"] == 0


@pytest.mark.parametrize("image, want", [
    (b"", gm.OK),
    (b"\0" * 17, gm.INVALID_BUFFER),
    (b"\0" * 18, gm.GZIP_ID),
    (b"\x1f\x8b\x07" + b"\0" * 15, gm.UNSUPPORTED_METHOD),
    (b"\x1f\x8b\x08\x20" + b"\0" * 14, gm.RESERVED_FLAGS),
    (b"\x1f\x8b\x08\x04" + b"\0" * 6 + b"\xff\xff" + b"\0" * 30, gm.INVALID_BUFFER),
    (b"\x1f\x8b\x08\x08" + b"\0" * 6 + b"x" * 30, gm.INVALID_BUFFER),
    (b"\x1f\x8b\x08\x10" + b"\0" * 6 + b"x" * 30, gm.INVALID_BUFFER),
    (b"\x1f\x8b\x08\x0a" + b"\0" * 6 + b"x" * 7 + b"\0", gm.INVALID_BUFFER),
    (gc.member(b"abc", crc=1), gm.CHECKSUM),
    (gc.member(b"abc", isize=4), gm.SIZE),
    (gc.member(b"abc", crc=1, isize=4), gm.CHECKSUM),
    (gc.member(b"abc", name=b"n", hcrc=True, hcrc_xor=1, crc=1), gm.CHECKSUM),
    (gc.member(b"abc")[:-1], REFUSED),
    (gc.member(b"abc") + b"\x01", gm.INVALID_BUFFER),
    (gc.member(b"abc") + b"\0" * 9, gm.OK),
    (gc.member(b"abc") + b"\0" * 20 + b"\x01", gm.GZIP_ID),
    (gc.member(b"abc") + gc.member(b"def", isize=9), gm.SIZE),
])
def test_model_check_order(image, want):
    assert gm.read(image, refuse)[0] == want


def test_model_accepts_the_adversarial_image():
    gc.check_adversarial_model()
