"""The host side of zh_tar_read_batch (zh_tar_read_batch.hip's driver, zh_tar_dev.h, zh_tar.hip) under
AddressSanitizer and UndefinedBehaviorSanitizer: zippy_amd/csrc built by g++ against the emulator runtime of
tests/hipemu and linked with tests/tar_read_sanitize_main.cpp into a stand-alone program (tests/sanitize_build.py), which opens the cases of
tests/tar_read_cases.py (the chains up to 600 blocks) -- each by itself and all in one call -- and holds the statuses
against the model's.  Nothing is built under the tree."""
import tar_read_cases as rc
import sanitize_build


def test_tar_read_host_code_under_sanitizers(tmp_path):
    cases = [x for x in rc.all_cases() if len(x[1]) <= 600 * 512]
    assert rc.dump(str(tmp_path / "cases"), cases) > 250
    r = sanitize_build.run_main("tar_read_sanitize_main.cpp", str(tmp_path / "cases"), tmp_path)
    sanitize_build.assert_clean(r, "sanitized tar read ok")
