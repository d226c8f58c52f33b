"""The BestSpeed matcher under AddressSanitizer and UndefinedBehaviorSanitizer: zippy_amd/csrc built by g++ against
the emulator runtime of tests/hipemu and linked with tests/l1_ahead_sanitize_main.cpp into a stand-alone program
(tests/sanitize_build.py).  The emulator's device allocations are plain malloc blocks, which the sanitizer guards: the
program compresses the tail family (every length 0 .. 300, 32 768 - k) and the boundary family of l1_ahead_cases, each
input in an allocation of its own that ends with the dword holding its last byte, 0 .. 3 bytes behind the allocation's
start -- no load of the matcher, asked for early or not, may pass it.  The matcher's aligned-dword source reads reach
the end of the last byte's dword by design (zh_l1_match.hip), so an allocation ends with that dword; for every length
one of the four misalignments makes that the last byte itself.  Nothing is built under the tree."""
import os

import l1_ahead_cases as lc
import oracle
import sanitize_build
import synth


def test_l1_match_under_sanitizers(tmp_path):
    cases = lc.t_cases(synth.corpus_file("alice29.txt")) + lc.b_cases()
    d = tmp_path / "cases"
    os.makedirs(d / "expected")
    names = []
    for i, (name, src) in enumerate(cases):
        names.append("c%05d" % i)
        (d / names[-1]).write_bytes(src)
        (d / "expected" / names[-1]).write_bytes(oracle.deflate(src, 1))
    (d / "list.txt").write_text("\n".join(names) + "\n")
    assert len(names) > 2500
    r = sanitize_build.run_main("l1_ahead_sanitize_main.cpp", str(d), tmp_path)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "sanitized l1 match ok: %d inputs x 4 misalignments" % len(names) in r.stdout
    assert "AddressSanitizer" not in r.stderr
    for line in r.stderr.splitlines():  # UBSan reports do not stop the program: none may name the matcher
        assert not ("runtime error" in line and "zh_l1_match" in line), line
