"""Cases of the zip writers that tests/test_emu_zip_write.py (the emulator), tests/test_gpu_zip_write.py (the device)
and tests/test_zip_write_sanitize.py (the stand-alone sanitized program) run, against tests/zip_v1_writer_model.py and
tests/zip_v2_writer_model.py."""
import os

import zip_v1_writer_model as zm
import zip_v2_writer_model as z2

SIZES = [0, 1, 3, 4, 15, 16, 17, 140000]
T, D = 0x6000, 0x5521


def blob(n, seed=1):
    return bytes((i * 131 + seed * 7 + (i >> 7) + (i * i >> 11)) & 0xFF for i in range(n))


def check_end_record_alignments(eng):
    """The 22-byte end record is a task of its own.  One call at level 0: sixteen one-entry archives without contents,
    path lengths 1..16 -- the end record alone in its archive, at 76 + 2 * plen: the even residues mod 16 --; the same
    sixteen with two bytes of contents, a stored stream of 7 bytes: the odd residues; and one archive whose last
    entry's stream is longer than a slice (32 768 bytes), so that the end record follows an entry of two tasks."""
    zips = [[("p" * plen, contents)] for contents in (b"", b"xy") for plen in range(1, 17)]
    zips.append([("small", b"s"), ("big", blob(40000))])
    want = [zm.image(z, 0) for z in zips]
    ends = [len(w) - 22 for w in want]
    assert all(w[e:e + 4] == b"PK\x05\x06" for w, e in zip(want, ends))
    assert {e % 16 for e in ends[:32]} == set(range(16))
    assert int.from_bytes(want[32][-22 - 46 - 3 + 20:-22 - 46 - 3 + 24], "little") > 32768  # "big"'s stream
    outs, sts = eng.write_zips(zips, 0)
    assert sts == [0] * 33
    for k, (out, w) in enumerate(zip(outs, want)):
        assert out == w, k


# the sanitized program's calls: the entry sizes; an empty archive, a duplicate, a name of 65 536 bytes, good and bad mixed
CALLS = {
    "sizes": [[("f%d.bin" % n, blob(n, n)) for n in SIZES]],
    "mixed": [[("one.txt", b"hello")], [], [("a", b"1"), ("b", b"2"), ("a", b"")], [("x" * 65536, b"")],
              [("d/", (b"", True)), ("d/x", blob(1000, 3))], [("d/", b"x")], [("", b"x"), ("ok", b"y")], [("/abs", b"z")]],
}


def dump(path):
    """CALLS as tests/zip_write_sanitize_main.cpp reads them -> {(call, form, archive): (status, image or None)}, the
    models' answers for zh_zip_write_batch (v1), zh_zip_create_batch (v2) and zh_zip_create (one)"""
    os.makedirs(path)
    want = {}
    with open(os.path.join(path, "calls.txt"), "w") as calls:
        for name, zips in CALLS.items():
            rows = [(t,) + e for t, z in enumerate(zips) for e in zm.normalize(z)]
            calls.write("%s %d %d %d %d\n" % (name, len(zips), len(rows), T, D))
            with open(os.path.join(path, name + ".tab"), "w") as f:
                f.write("".join("%d %d\n" % (t, is_dir) for t, _, _, is_dir, _, _ in rows))
            for k, (_, p, contents, _, _, _) in enumerate(rows):
                for ext, data in ((".path", p), (".data", contents)):
                    with open(os.path.join(path, "%s_%d%s" % (name, k, ext)), "wb") as f:
                        f.write(data)
            for t, z in enumerate(zips):
                v1 = [(p, (c, d, T, D)) for p, c, d, _, _ in zm.normalize(z)]
                v2 = [(p, c) for p, c, _, _, _ in zm.normalize(z)]
                want[name, "v1", t] = (zm.status(v1), None if zm.status(v1) else zm.image(v1))
                want[name, "v2", t] = want[name, "one", t] = (z2.status(v2), None if z2.status(v2) else z2.image(v2, T, D))
    return want


def load(path):
    """what the program wrote back, in dump's form"""
    got = {}
    with open(os.path.join(path, "out.txt")) as f:
        for line in f.read().splitlines():
            name, form, t, st, _ = line.split()
            img = os.path.join(path, "%s.%s.%s.img" % (name, form, t))
            got[name, form, int(t)] = (int(st), open(img, "rb").read() if os.path.exists(img) else None)
    return got
