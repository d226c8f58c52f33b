"""zh_bgzf_write_batch, zh_bgzf_read_batch, zh_bgzf_index_batch and zh_bgzf_read_ranges (zippy_amd/csrc/zh_bgzf.hip, host
code and kernels) under AddressSanitizer and UndefinedBehaviorSanitizer: zippy_amd/csrc built by g++ against the
emulator runtime of tests/hipemu and linked with tests/bgzf_sanitize_main.cpp into a stand-alone program
(tests/sanitize_build.py), which drives all four calls over the dumped cases of tests/bgzf_cases.py and holds bytes
and statuses against the model's."""
import bgzf_cases as bc
import sanitize_build


def test_bgzf_under_sanitizers(tmp_path):
    n_write, n_read, n_ranges = bc.dump(str(tmp_path / "cases"))
    assert n_write > 40 and n_read > 35 and n_ranges > 60
    r = sanitize_build.run_main("bgzf_sanitize_main.cpp", str(tmp_path / "cases"), tmp_path)
    sanitize_build.assert_clean(r, "sanitized bgzf ok")
    for line in r.stderr.splitlines():  # (assert_clean's filter does not know the new files' names)
        assert not ("runtime error" in line and any(x in line for x in ("zh_bgzf", "zh_scan", "zh_range_host"))), line
