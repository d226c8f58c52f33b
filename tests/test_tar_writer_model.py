"""CPU checks of tests/tar_writer_model.py, the restatement of writeTarball (tarballs_v1.nim:203-261) that the
device tests compare against: one header pinned byte for byte, and images read back by Python's tarfile and by
the restatement of the reference's reader (oracle/tar_oracle.py)."""
import io
import tarfile

import pytest

import tar_writer_model as twm


def _z(n):
    return b"\0" * n


# writeTarball's header of ("README.txt", "Hello, World!", ekNormalFile, fromUnix(1600000000)), field by field
PINNED = (b"README.txt" + _z(90)          # 0-99 name
          + b"000777 \0"                  # 100-107 mode
          + b"000000 \0" + b"000000 \0"   # 108-123 uid, gid
          + b"00000000015 "               # 124-135 size 13
          + b"13727410000 "               # 136-147 mtime 1600000000
          + b"010717\0 "                  # 148-155 checksum 4559
          + b"0" + _z(100)                # 156 kind, 157-256 linkname
          + b"ustar\0" + b"00" + _z(64)   # 257-328
          + b"000000\0 " + b"000000\0 "   # 329-344 devmajor, devminor
          + _z(167))                      # 345-511 prefix (empty) and the rest


def test_pinned_header():
    assert len(PINNED) == 512
    img = twm.image([("README.txt", (b"Hello, World!", "0", 1600000000))])
    assert img[:512] == PINNED
    assert img[512:525] == b"Hello, World!" and img[525:] == bytes(len(img) - 525)
    assert len(img) == 512 + 512 + 1024


@pytest.mark.parametrize("path,head,tail", [
    (b"README.txt", b"", b"README.txt"), (b"/bin", b"/", b"bin"), (b"a/b/", b"a/b", b""), (b"a//b", b"a/", b"b"),
    (b"x/y/z.txt", b"x/y", b"z.txt"), (b"/", b"/", b""),
])
def test_split_path(path, head, tail):
    assert twm.split_path(path) == (head, tail)


def _sample():
    return [("README.txt", (b"Hello, World!", "0", 1600000000)),
            ("docs", (b"", "5", 1234567890)),
            ("docs/guide.md", b"# guide\n" * 100),
            ("docs/empty", b""),
            ("data/" + "d" * 140 + "/blob.bin", (bytes(range(256)) * 9, "0", 7)),
            ("n" * 99, b"x" * 512)]


def test_image_reads_back_with_tarfile():
    entries = _sample()
    img = twm.image(entries)
    assert len(img) % 512 == 0 and img.endswith(bytes(1024))
    with tarfile.open(fileobj=io.BytesIO(img), mode="r:") as tf:
        members = tf.getmembers()
        assert [m.name for m in members] == [p for p, _ in entries]
        for m, (_, v) in zip(members, entries):
            contents, kind, mtime = v + ("0", 0)[len(v) - 1:] if isinstance(v, tuple) else (v, "0", 0)
            assert m.size == len(contents) and m.mtime == mtime and m.mode == 0o777
            assert m.type == kind.encode()
            if kind == "0":
                assert tf.extractfile(m).read() == contents


def test_image_reads_back_with_the_reference_reader():
    from oracle import tar_oracle
    entries = _sample()
    img = twm.image(entries)
    data, got = tar_oracle.open_tarball(img)
    assert data == img
    assert [e["path"] for e in got] == [p.encode() for p, _ in entries]
    assert [e["size"] for e in got] == [len(v[0] if isinstance(v, tuple) else v) for _, v in entries]
    assert [e["typeflag"] for e in got] == [b"0", b"5", b"0", b"0", b"0", b"0"]


def test_model_statuses():
    assert twm.status([]) == twm.ZH_ERR_TAR_EMPTY
    assert twm.status([("a" * 154 + "/x", b"")]) == 0
    assert twm.status([("a" * 155 + "/x", b"")]) == twm.ZH_ERR_TAR_PATH
    assert twm.status([("t" * 99, b"")]) == 0
    assert twm.status([("t" * 100, b"")]) == twm.ZH_ERR_TAR_NAME
    assert twm.status([("a" * 155 + "/" + "t" * 100, b"")]) == twm.ZH_ERR_TAR_PATH  # head is checked first
    assert twm.status([("a", (b"", "2", 0))]) == twm.ZH_ERR_ARGUMENT
    assert twm.status([("a", (b"", "0", -1))]) == twm.ZH_ERR_ARGUMENT
    assert twm.status([("a", (b"", "0", 8 ** 11))]) == twm.ZH_ERR_ARGUMENT
    assert twm.status([("a", (b"", "0", 8 ** 11 - 1))]) == 0
    assert twm.status([("a", b"1"), ("b", b"2"), ("a", b"3")]) == twm.ZH_ERR_ARGUMENT
    # the first failing entry decides
    assert twm.status([("a", b""), ("t" * 100, b""), ("a" * 155 + "/x", b"")]) == twm.ZH_ERR_TAR_NAME
