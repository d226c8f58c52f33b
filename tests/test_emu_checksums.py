"""CPU-only: the checksum cases of tests/parity_cases.py (csrc/zh_checksum.hip against zlib.crc32 / zlib.adler32) on
the emulator build of the kernel sources, in the subsets the emulator can afford; tests/test_gpu_checksums.py runs
them whole on an MI355X."""
import ctypes

import pytest

import emu
import parity_cases as pc


@pytest.fixture(scope="module")
def eng():
    return emu.engine()


def _upload(b):
    buf = ctypes.create_string_buffer(b, len(b))
    return ctypes.addressof(buf), buf


def _alloc(n, fill):
    buf = ctypes.create_string_buffer(bytes([fill]) * n, n)
    return ctypes.addressof(buf), buf


def _download(keep):
    return keep.raw


def test_emu_checksum_lengths(eng):
    """The whole case: nothing is left out."""
    pc.check_checksum_lengths(eng)


def test_emu_checksum_alignment(eng):
    """The whole case (the emulator takes a quarter of a minute for it): nothing is left out."""
    pc.check_checksum_alignment(eng, _upload, _download, _alloc)


def test_emu_checksum_uncompress(eng):
    """Left out: output alignments 2..14 (0, 1 and 15 run: no head, the longest and the shortest one), the lengths
    between 6200 and 32768, around 34816 and 65536, and 98305 (32768, 32769 and 65537 run); the three fills take turns
    stream by stream instead of the random and the 0xFF fill running whole (three minutes here)."""
    pc.check_checksum_uncompress(eng, _upload, _download, _alloc, small=True)


def test_emu_checksum_piece_counts(eng):
    """The whole case: nothing is left out."""
    pc.check_checksum_piece_counts(eng, _upload, _download, _alloc)


def test_emu_checksum_entry_points(eng):
    """The whole case: nothing is left out."""
    pc.check_checksum_entry_points(eng)
