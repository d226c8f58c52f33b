"""CPU-only checks of the resumable uncompress at the C boundary and in the Python interface: the hipcc-built library
exports the entry point and refuses a NULL context without touching a device; the state header's size, offsets and the
enum values are include/zippy_hip.h's; api.Inflater and api.uncompress_chunks exist with their arguments."""
import ctypes as c
import inspect
import os

import subprocess

import pytest

import resume_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resume_symbol_exported_and_null_context():
    from zippy_amd import build, _binding
    lib = _binding.load_library(build.build())
    assert "zh_uncompress_resume_batch" in _binding.EXPORTED_SYMBOLS
    st = (c.c_int32 * 1)(5)
    assert lib.zh_uncompress_resume_batch(None, None, None, 0, 0, None, None, None, None, None, None, None, None, None,
                                          None, st) == 22
    assert st[0] == 5  # (nothing was touched)


def test_resume_header_layout(tmp_path):
    """the struct as a C compiler lays it out, against the model's format string"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zippy_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %s %u %d %d %d\\n", sizeof(zh_resume_header),\n'
                   '         offsetof(zh_resume_header, magic), offsetof(zh_resume_header, version),\n'
                   '         offsetof(zh_resume_header, data_format), offsetof(zh_resume_header, phase),\n'
                   '         offsetof(zh_resume_header, bit_skip), offsetof(zh_resume_header, total_in),\n'
                   '         offsetof(zh_resume_header, total_out), offsetof(zh_resume_header, check),\n'
                   '         offsetof(zh_resume_header, win_len), offsetof(zh_resume_header, reserved), ZH_RESUME_MAGIC,\n'
                   '         ZH_RESUME_VERSION, ZH_RESUME_DONE, ZH_RESUME_NEED_INPUT, ZH_RESUME_NEED_OUTPUT);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["64", "0", "8", "12", "16", "20", "24", "32", "40", "44", "48", "ZHRESUM1", "1", "0", "1", "2"]
    assert rm.STATE.size == 64 and rm.MAGIC == b"ZHRESUM1" and (rm.DONE, rm.NEED_INPUT, rm.NEED_OUTPUT) == (0, 1, 2)
    blob = rm.pack_state(2, 1, 5, 0x1122334455, 0x66778899aa, 0xdeadbeef, b"w" * 7)
    assert blob[12:16] == b"\2\0\0\0" and blob[20] == 5 and blob[24:29] == bytes.fromhex("5544332211")
    assert blob[40:44] == bytes.fromhex("efbeadde") and blob[44] == 7 and blob[48:64] == bytes(16) and blob[64:] == b"w" * 7


def test_resume_python_interface():
    from zippy_amd import api
    assert list(inspect.signature(api.Inflater.__init__).parameters)[1:] == ["fmt", "max_out"]
    assert list(inspect.signature(api.Inflater.feed).parameters)[1:] == ["chunk", "last"]
    assert inspect.isgeneratorfunction(api.uncompress_chunks)
    assert list(inspect.signature(api.uncompress_resume_batch).parameters) == ["srcs", "states", "max_out", "last",
                                                                               "dataFormat"]


def test_resume_nim_binding_and_docs_name_it():
    nim = open(os.path.join(ROOT, "bindings", "nim", "hip.nim")).read()
    assert "zh_uncompress_resume_batch" in nim and "hipUncompressResume" in nim
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "zh_uncompress_resume_batch" in open(os.path.join(ROOT, doc)).read(), doc
