"""zh_seek_index_batch and zh_seek_read_ranges (zippy_amd/csrc/zh_seek.hip, the recording and seek forms of the
inflate kernels, the host arithmetic of zh_range_host.h) under AddressSanitizer and UndefinedBehaviorSanitizer:
zippy_amd/csrc built by g++ against the emulator runtime of tests/hipemu and linked with tests/seek_main.cpp into a
stand-alone program (tests/sanitize_build.py), which builds the indexes of the dumped cases of tests/seek_cases.py,
holds them against the model's blobs byte for byte, and reads the dumped ranges -- sound, damaged and statically
unsound blobs, points at every block start, a forged window one byte short whose slot is the scratch's first, a clean
decode of the wrong length -- against statuses and slices."""
import sanitize_build
import seek_cases as sc


def test_seek_under_sanitizers(tmp_path):
    n_cases, n_ranges = sc.dump(str(tmp_path / "cases"))
    assert n_cases == 10 and n_ranges > 85
    r = sanitize_build.run_main("seek_main.cpp", str(tmp_path / "cases"), tmp_path)
    sanitize_build.assert_clean(r, "sanitized seek ok")
    for line in r.stderr.splitlines():  # (assert_clean's filter does not know these files' names)
        assert not ("runtime error" in line and any(x in line for x in ("zh_seek", "zh_range_host", "zh_inflate"))), line
