"""The host side of zh_zip_read_batch (zh_zip_read_batch.hip's driver, zh_zip.hip) under AddressSanitizer and
UndefinedBehaviorSanitizer: zippy_amd/csrc built by g++ against the emulator runtime of tests/hipemu and linked with
tests/zip_read_sanitize_main.cpp into a stand-alone program (tests/sanitize_build.py), which opens the scan geometry, straddling, decoy, status,
table and alignment cases of tests/zip_read_cases.py and the chains up to 2^8 + 1 local records -- each by itself and
all in one call -- and holds the statuses against the model's."""
import zip_read_cases as zc
import sanitize_build


def test_zip_read_host_code_under_sanitizers(tmp_path):
    cases = (zc.scan_geometry() + zc.straddling_pair() + zc.decoys() + zc.statuses() + zc.tables()
             + [x for x in zc.chains() if len(x[1]) <= 46 * 2 * 257 + 22] + [("alignment", zc.alignment(), 0)])
    assert zc.dump(str(tmp_path / "cases"), cases) > 150
    r = sanitize_build.run_main("zip_read_sanitize_main.cpp", str(tmp_path / "cases"), tmp_path)
    sanitize_build.assert_clean(r, "sanitized zip read ok")
