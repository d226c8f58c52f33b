"""CPU-only checks of the seek-index entry points at the C boundary: the hipcc-built library exports them and refuses a
NULL context without touching a device; under the emulator, NULL arrays and empty calls behave as include/zippy_hip.h
says."""
import ctypes as c

import pytest


@pytest.fixture(scope="module")
def lib():
    from zippy_amd import build, _binding
    return _binding.load_library(build.build())


def test_seek_symbols_exported_and_null_context(lib):
    from zippy_amd import _binding
    for name in ("zh_seek_index_batch", "zh_seek_read_ranges"):
        assert name in _binding.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    st = (c.c_int32 * 1)(5)
    assert lib.zh_seek_index_batch(None, None, None, 0, 2, 0, None, None, None, None, st) == 22
    assert lib.zh_seek_read_ranges(None, None, None, 0, None, None, 0, None, None, None, None, None, st) == 22
    assert st[0] == 5  # (nothing was touched)


def test_seek_null_arguments_and_empty_calls():
    import emu
    eng = emu.engine()
    lib, h = eng.lib, eng._h
    one = (c.c_uint64 * 1)(0)
    src = (c.c_void_p * 1)(c.cast(c.c_char_p(b"xyz"), c.c_void_p))
    n3 = (c.c_size_t * 1)(3)
    out, olen, st = (c.c_void_p * 1)(1), (c.c_size_t * 1)(7), (c.c_int32 * 1)(5)
    # n == 0: nothing runs, whatever the arrays
    assert lib.zh_seek_index_batch(h, None, None, 0, 2, 0, None, None, None, None, None) == 0
    assert lib.zh_seek_read_ranges(h, None, None, 0, None, None, 0, None, None, None, None, None, None) == 0
    # NULL arrays with something to do
    assert lib.zh_seek_index_batch(h, None, n3, 1, 2, 0, out, olen, None, None, st) == 22
    assert lib.zh_seek_index_batch(h, src, n3, 1, 2, 0, None, olen, None, None, st) == 22
    assert lib.zh_seek_index_batch(h, src, n3, 1, 2, 0, out, olen, out, None, st) == 22  # (dsts without dst_lens)
    assert lib.zh_seek_read_ranges(h, src, n3, 1, None, None, 1, one, one, one, out, olen, st) == 22
    assert lib.zh_seek_read_ranges(h, src, n3, 1, src, n3, 1, None, one, one, out, olen, st) == 22
    assert lib.zh_seek_read_ranges(h, src, n3, 1, src, n3, 1, one, one, one, None, olen, st) == 22
    # a bad format: every stream's status and the call's, as in zh_uncompress_batch; a span below the window
    assert lib.zh_seek_index_batch(h, src, n3, 1, 9, 0, out, olen, None, None, st) == 2 and st[0] == 2 and not out[0]
    assert lib.zh_seek_index_batch(h, src, n3, 1, 2, 32767, out, olen, None, None, st) == 22
    # a stream that is no stream: its status, NULL / 0, and the call succeeds
    assert lib.zh_seek_index_batch(h, src, n3, 1, 2, 0, out, olen, None, None, st) == 0
    assert st[0] != 0 and not out[0] and olen[0] == 0
