"""The typed arena of zippy_amd/csrc/zh_host.h (every device array of a plan or a batch call is declared through it)
under AddressSanitizer and UndefinedBehaviorSanitizer: tests/arena_sanitize_main.cpp drives it directly, built by g++
against the emulator runtime of tests/hipemu into a stand-alone program (tests/sanitize_build.py).  Offsets, the total,
empty arrays, uploads and an arena of nothing.  Nothing is built under the tree."""
import sanitize_build


def test_arena_under_sanitizers(tmp_path):
    r = sanitize_build.run_main("arena_sanitize_main.cpp", str(tmp_path), tmp_path)
    sanitize_build.assert_clean(r, "sanitized arena ok")
