"""CPU-only: zh_gzip_member as include/zippy_hip.h declares it against its ctypes mirror (zippy_amd/_binding.py) -- the
header's struct is compiled by the host compiler, its size and every field's offset must be the mirror's -- and the two
entry points in the built library."""
import os
import re
import subprocess

from zippy_amd import _binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gzip_member_layout(tmp_path):
    fields = [name for name, _ in _binding.GzipMember._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "zippy_hip.h"\nint main(void) {\n'
                   '  printf("sizeof %zu\\n", sizeof(zh_gzip_member));\n' +
                   "".join('  printf("%s %%zu\\n", offsetof(zh_gzip_member, %s));\n' % (f, f) for f in fields) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got.pop("sizeof")) == _binding.ctypes.sizeof(_binding.GzipMember) == 80
    assert {k: int(v) for k, v in got.items()} == {f: getattr(_binding.GzipMember, f).offset for f in fields}
    hdr = open(os.path.join(ROOT, "include", "zippy_hip.h")).read()
    body = re.search(r"typedef struct zh_gzip_member \{(.*?)\} zh_gzip_member;", hdr, flags=re.S).group(1)
    declared = re.findall(r"\b([a-z_]+)\s*[,;]", body)
    assert declared == fields


def test_gzip_entry_points_exported():
    from zippy_amd import build
    lib = _binding.load_library(build.build())
    assert lib.zh_gzip_read_batch is not None and lib.zh_debug_gzip_stats is not None
    assert "zh_gzip_read_batch" in _binding.EXPORTED_SYMBOLS and "zh_debug_gzip_stats" in _binding.EXPORTED_SYMBOLS
