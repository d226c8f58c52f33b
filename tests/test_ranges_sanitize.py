"""zh_uncompress_ranges and zh_plan_uncompress_ranges + zh_plan_run (zippy_amd/csrc/zh_ranges.hip and the host
arithmetic it shares with zh_bgzf.hip, zh_range_host.h) under AddressSanitizer and UndefinedBehaviorSanitizer:
zippy_amd/csrc built by g++ against the emulator runtime of tests/hipemu and linked with tests/ranges_sanitize_main.cpp
into a stand-alone program (tests/sanitize_build.py), which drives both forms over the dumped cases of
tests/ranges_cases.py -- streams and indexes from the oracle -- and holds statuses, bytes and the upload's size against
them."""
import ranges_cases as rc
import sanitize_build


def test_ranges_under_sanitizers(tmp_path):
    n_cases, n_ranges = rc.dump(str(tmp_path / "cases"))
    assert n_cases == 1 + 1 + 6 + 5 and n_ranges > 130
    r = sanitize_build.run_main("ranges_sanitize_main.cpp", str(tmp_path / "cases"), tmp_path)
    sanitize_build.assert_clean(r, "sanitized ranges ok")
    for line in r.stderr.splitlines():  # (assert_clean's filter does not know these files' names)
        assert not ("runtime error" in line and any(x in line for x in ("zh_ranges", "zh_range_host", "zh_scan"))), line
