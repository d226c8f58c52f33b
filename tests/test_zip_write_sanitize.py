"""zh_zip_write_batch, zh_zip_create_batch and zh_zip_create (zh_zip_write.hip's one driver and one kernel body,
zh_gather.h's range copy, zh_zip.hip's single-archive call) under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/zip_write_sanitize_main.cpp as a stand-alone program (tests/sanitize_build.py) over tests/zip_write_cases.py's
calls, with ZH_COMPRESS_FIRST_CAP=64, so that the larger contents are compressed twice; held against the models."""
import sanitize_build
import zip_write_cases as zc


def test_zip_writers_under_sanitizers(tmp_path, monkeypatch):
    want = zc.dump(str(tmp_path / "cases"))
    assert {st for st, _ in want.values()} == {0, 22, 31, 33, 40, 41}  # ARGUMENT, DUPLICATE, NAME, EMPTY, TOO_LARGE
    monkeypatch.setenv("ZH_COMPRESS_FIRST_CAP", "64")
    r = sanitize_build.run_main("zip_write_sanitize_main.cpp", str(tmp_path / "cases"), tmp_path)
    sanitize_build.assert_clean(r, "sanitized zip writers ok")
    assert zc.load(str(tmp_path / "cases")) == want
