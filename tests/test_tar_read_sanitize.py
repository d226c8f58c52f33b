"""The host side of zh_tar_read_batch (zh_tar_read_batch.hip's driver, zh_tar_dev.h, zh_tar.hip) under
AddressSanitizer and UndefinedBehaviorSanitizer: zippy_amd/csrc built by g++ against the emulator runtime of
tests/hipemu and linked with tests/tar_read_sanitize_main.cpp into a stand-alone program, which opens the cases of
tests/tar_read_cases.py (the chains up to 600 blocks) -- each by itself and all in one call -- and holds the statuses
against the model's.  Nothing is built under the tree."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import tar_read_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-w"]


def test_tar_read_host_code_under_sanitizers(tmp_path):
    from zippy_amd.build import SOURCES
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                           input="int main() { return 0; }", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("no sanitizer runtime in this toolchain")
    emu_dir = os.path.join(ROOT, "tests", "hipemu")
    jobs, objs = [], []
    for src in SOURCES:
        objs.append(str(tmp_path / (src[:-4] + ".o")))
        jobs.append(["g++"] + FLAGS + ["-x", "c++", "-I", emu_dir, "-c", os.path.join(ROOT, "zippy_amd", "csrc", src),
                                       "-o", objs[-1]])
    for src in (os.path.join(emu_dir, "emu.cpp"), os.path.join(ROOT, "tests", "tar_read_sanitize_main.cpp")):
        objs.append(str(tmp_path / (os.path.basename(src)[:-4] + ".o")))
        jobs.append(["g++"] + FLAGS + ["-I", emu_dir, "-c", src, "-o", objs[-1]])
    with ThreadPoolExecutor(max_workers=8) as ex:
        for r in ex.map(lambda cmd: subprocess.run(cmd, capture_output=True, text=True), jobs):
            assert r.returncode == 0, r.stderr[-3000:]
    exe = str(tmp_path / "tar_read_san")
    subprocess.run(["g++", "-fsanitize=address,undefined", "-o", exe] + objs + ["-lpthread"], check=True)
    cases = [x for x in rc.all_cases() if len(x[1]) <= 600 * 512]
    assert rc.dump(str(tmp_path / "cases"), cases) > 250
    # (the emulator keeps its fibers' stacks for the life of the process: no leak check)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:detect_stack_use_after_return=0",
               UBSAN_OPTIONS="print_stacktrace=1", ZH_PIN_CHUNK="131072", ZH_HOST_THREADS="3")
    r = subprocess.run([exe, str(tmp_path / "cases")], capture_output=True, text=True, env=env, timeout=1200)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "sanitized tar read ok" in r.stdout
    assert "AddressSanitizer" not in r.stderr
    for line in r.stderr.splitlines():  # UBSan reports do not stop the program: none may name the new code
        assert not ("runtime error" in line and ("zh_tar" in line or "zh_walk" in line)), line
