"""zh_gzip_read_batch (zippy_amd/csrc/zh_gzip.hip, the speculative sizing form of the tokens kernel, the scan and the
walk it shares with the other readers) under AddressSanitizer and UndefinedBehaviorSanitizer: zippy_amd/csrc built by
g++ against the emulator runtime of tests/hipemu and linked with tests/gzip_main.cpp into a stand-alone program
(tests/sanitize_build.py), which reads the dumped cases of tests/gzip_cases.py -- chains, stream ends, every header
field, false candidates, tails and cuts, signatures astride chunks and images, each with the default budget and with
none at all, and candidates and unterminated names that exhaust a small one -- against the model's statuses, data and member records."""
import gzip_cases as gc
import sanitize_build


def test_gzip_under_sanitizers(tmp_path):
    n_cases, n_images = gc.dump(str(tmp_path / "cases"))
    assert n_cases == 14 and n_images > 120
    r = sanitize_build.run_main("gzip_main.cpp", str(tmp_path / "cases"), tmp_path)
    sanitize_build.assert_clean(r, "sanitized gzip ok")
    for line in r.stderr.splitlines():  # (assert_clean's filter does not know these files' names)
        assert not ("runtime error" in line and any(x in line for x in ("zh_gzip", "zh_range_host", "zh_inflate"))), line
