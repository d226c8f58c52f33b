"""The host side of zh_zip_open_all_batch (zh_zip_open_batch.hip's driver, zh_zip.hip) under AddressSanitizer and
UndefinedBehaviorSanitizer: zippy_amd/csrc built by g++ against the emulator runtime of tests/hipemu and linked with
tests/zip_open_sanitize_main.cpp into a stand-alone program (tests/sanitize_build.py), which opens the status, precedence, entry, name,
geometry and zip64 cases of tests/zip_open_cases.py -- each by itself and all in one call -- and holds the archive
statuses against the oracle's and zh_zip_open's."""
import zip_open_cases as zc
import sanitize_build


def test_zip_open_host_code_under_sanitizers(tmp_path):
    assert zc.dump(str(tmp_path / "cases")) > 100
    r = sanitize_build.run_main("zip_open_sanitize_main.cpp", str(tmp_path / "cases"), tmp_path)
    sanitize_build.assert_clean(r, "sanitized zip open ok")
