"""zh_uncompress_resume_batch (zippy_amd/csrc/zh_resume.hip, the resuming form of the wave-pair inflate) under
AddressSanitizer and UndefinedBehaviorSanitizer: zippy_amd/csrc built by g++ against the emulator runtime of
tests/hipemu and linked with tests/resume_main.cpp into a stand-alone program (tests/sanitize_build.py), which replays
the dumped calls of tests/resume_cases.py -- every prefix of the small stream, the budgets, the window's edge with the
forged state one byte short, damaged trailers and states, the batch of 33 -- from exact-size heap copies and holds every
answer against the model's byte for byte."""
import os

import resume_cases as rc
import sanitize_build


def test_resume_under_sanitizers(tmp_path):
    os.makedirs(tmp_path / "cases")
    calls, streams = rc.dump(str(tmp_path / "cases" / "cases.bin"))
    assert calls > 20 and streams > 2000
    r = sanitize_build.run_main("resume_main.cpp", str(tmp_path / "cases"), tmp_path)
    sanitize_build.assert_clean(r, "sanitized resume ok")
    for line in r.stderr.splitlines():  # (assert_clean's filter does not know these files' names)
        assert not ("runtime error" in line and any(x in line for x in ("zh_resume", "zh_range_host", "zh_inflate"))), line
