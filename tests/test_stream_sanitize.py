"""zh_compress_stream_batch (zippy_amd/csrc/zh_stream.hip: the host call, zh_stream_consts_kernel and
zh_stream_splice_kernel with zh_gather.h's gathers) under AddressSanitizer and UndefinedBehaviorSanitizer:
zippy_amd/csrc built by g++ against the emulator runtime of tests/hipemu and linked with tests/stream_main.cpp into a
stand-alone program (tests/sanitize_build.py), which replays the dumped calls of tests/stream_cases.py -- the covering few
of the alignment family, the stored and empty families, lengths around a block, damaged states, the batch of 33 -- from
exact-size heap copies and holds every answer against the model's byte for byte."""
import os

import sanitize_build
import stream_cases as sc


def test_stream_under_sanitizers(tmp_path):
    os.makedirs(tmp_path / "cases")
    calls, streams = sc.dump(str(tmp_path / "cases" / "cases.bin"))
    assert calls > 40 and streams > 300
    r = sanitize_build.run_main("stream_main.cpp", str(tmp_path / "cases"), tmp_path)
    sanitize_build.assert_clean(r, "sanitized stream ok")
    for line in r.stderr.splitlines():  # (assert_clean's filter does not know this file's name)
        assert not ("runtime error" in line and "zh_stream" in line), line
