"""CPU-only checks of the streaming compress at the C boundary and in the Python interface: the hipcc-built library
exports the entry point and refuses a NULL context without touching a device; the state's size, offsets and the enum
values are include/zippy_hip.h's; api.Deflater, api.compress_chunks and api.compress_stream_batch exist with their
arguments; the Nim shim and the documents name the call."""
import ctypes as c
import inspect
import os
import subprocess

import stream_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_symbol_exported_and_null_arguments():
    from zippy_amd import build, _binding
    lib = _binding.load_library(build.build())
    assert "zh_compress_stream_batch" in _binding.EXPORTED_SYMBOLS
    sig = _binding._SIGS["zh_compress_stream_batch"]
    assert sig[0] is c.c_int and len(sig[1]) == 15 and sig[1][4:7] == [c.c_int, c.c_int, c.c_size_t]
    st = (c.c_int32 * 1)(5)
    assert lib.zh_compress_stream_batch(None, None, None, 0, 1, 2, 0, None, None, None, None, None, None, None, st) == 22
    assert lib.zh_compress_stream_batch(None, None, None, 1, 1, 2, 0, None, None, None, None, None, None, None, st) == 22
    assert st[0] == 5  # (nothing was touched)


def test_stream_state_layout(tmp_path):
    """the struct as a C compiler lays it out, against the model's format string"""
    fields = ("magic", "version", "data_format", "level", "block_bytes", "phase", "pend_bits", "pend_byte", "check",
              "total_in", "total_out", "reserved")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zippy_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(zh_stream_state));\n'
                   + "".join('  printf(" %%zu", offsetof(zh_stream_state, %s));\n' % f for f in fields)
                   + '  printf(" %s %u %d %d %d\\n", ZH_STREAM_MAGIC, ZH_STREAM_VERSION, ZH_FLUSH_BLOCK, ZH_FLUSH_SYNC,\n'
                   '         ZH_FLUSH_FINISH);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["64", "0", "8", "12", "16", "20", "24", "28", "32", "36", "40", "48", "56", "ZHCSTRM1", "1", "0", "1", "2"]
    assert sm.STATE.size == 64 and sm.MAGIC == b"ZHCSTRM1" and (sm.BLOCK, sm.SYNC, sm.FINISH) == (0, 1, 2)


def test_stream_python_interface():
    from zippy_amd import api
    assert list(inspect.signature(api.Deflater.__init__).parameters)[1:] == ["level", "dataFormat", "block_bytes"]
    assert list(inspect.signature(api.Deflater.feed).parameters)[1:] == ["piece", "flush"]
    assert inspect.signature(api.Deflater.feed).parameters["flush"].default == api.FLUSH_SYNC == 1
    assert list(inspect.signature(api.Deflater.finish).parameters)[1:] == ["piece"]
    assert inspect.isgeneratorfunction(api.compress_chunks)
    assert list(inspect.signature(api.compress_stream_batch).parameters) == ["srcs", "states", "flush", "level",
                                                                             "dataFormat", "block_bytes"]
    assert inspect.signature(api.compress_stream_batch).parameters["dataFormat"].default == api.dfGzip


def test_stream_nim_binding_and_docs_name_it():
    nim = open(os.path.join(ROOT, "bindings", "nim", "hip.nim")).read()
    assert "zh_compress_stream_batch" in nim and "hipCompressStream" in nim
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "zh_compress_stream_batch" in open(os.path.join(ROOT, doc)).read(), doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.19" in design and "a compress-side counterpart" not in design
