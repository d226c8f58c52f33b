"""The stand-alone sanitized programs of test_zip_open_sanitize.py, test_zip_read_sanitize.py,
test_tar_read_sanitize.py, test_zip_write_sanitize.py and test_arena_sanitize.py: zippy_amd/csrc built by g++ under AddressSanitizer and UndefinedBehaviorSanitizer against
the emulator runtime of tests/hipemu -- once a pytest process, into a temporary directory --, each test's main linked
against those objects and run directly.  Nothing is built under the tree."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "hipemu")
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-w"]
# the files of the batch readers: the calls' own, and the headers that hold what they share
READER_CODE = ("zh_zip", "zh_tar", "zh_walk", "zh_scan", "zh_gather", "zh_host")


def _compile(jobs):
    with ThreadPoolExecutor(max_workers=8) as ex:
        for r in ex.map(lambda cmd: subprocess.run(cmd, capture_output=True, text=True), jobs):
            assert r.returncode == 0, r.stderr[-3000:]


@functools.lru_cache(maxsize=None)
def _library_objects():
    """The library's sources and the emulator runtime as sanitized objects; None without a sanitizer runtime."""
    from zippy_amd.build import SOURCES
    out = tempfile.mkdtemp(prefix="zh_sanitize_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.path.join(out, "probe")],
                           input="int main() { return 0; }", capture_output=True, text=True)
    if probe.returncode != 0:
        return None
    jobs, objs = [], []
    for src in SOURCES:
        objs.append(os.path.join(out, src[:-4] + ".o"))
        jobs.append(["g++"] + FLAGS + ["-x", "c++", "-I", EMU_DIR, "-c", os.path.join(ROOT, "zippy_amd", "csrc", src),
                                       "-o", objs[-1]])
    objs.append(os.path.join(out, "emu.o"))
    jobs.append(["g++"] + FLAGS + ["-I", EMU_DIR, "-c", os.path.join(EMU_DIR, "emu.cpp"), "-o", objs[-1]])
    _compile(jobs)
    return tuple(objs)


def run_main(main_cpp, cases_dir, tmp_path):
    """tests/<main_cpp> linked against the sanitized library and run on the dumped cases; its CompletedProcess."""
    objs = _library_objects()
    if objs is None:
        pytest.skip("no sanitizer runtime in this toolchain")
    main_o, exe = str(tmp_path / "main.o"), str(tmp_path / main_cpp[:-len("_main.cpp")])
    _compile([["g++"] + FLAGS + ["-I", EMU_DIR, "-c", os.path.join(ROOT, "tests", main_cpp), "-o", main_o]])
    subprocess.run(["g++", "-fsanitize=address,undefined", "-o", exe, *objs, main_o, "-lpthread"], check=True)
    # (the emulator keeps its fibers' stacks for the life of the process: no leak check)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:detect_stack_use_after_return=0",
               UBSAN_OPTIONS="print_stacktrace=1", ZH_PIN_CHUNK="131072", ZH_HOST_THREADS="3")
    return subprocess.run([exe, cases_dir], capture_output=True, text=True, env=env, timeout=1200)


def assert_clean(r, ok_line):
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert ok_line in r.stdout
    assert "AddressSanitizer" not in r.stderr
    for line in r.stderr.splitlines():  # UBSan reports do not stop the program: none may name the readers' code
        assert not ("runtime error" in line and any(name in line for name in READER_CODE)), line
