"""The checksum kernels (csrc/zh_checksum.hip) on a real MI355X (-m gpu) against zlib.crc32 / zlib.adler32, which are
exact: every length, head alignment, piece count and entry point (the cases of tests/parity_cases.py, whole)."""
import pytest

import parity_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch  # torch's bundled HIP runtime has to initialise before libzippy_hip.so's
    torch.cuda.init()
    from zippy_amd import api
    e = api.engine()
    e.set_gzip_fname_len(0)
    return e


def _upload(b):
    import torch
    t = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    return t.data_ptr(), t


def _alloc(n, fill):
    import torch
    t = torch.full((n,), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t.data_ptr(), t


def _download(t):
    return t.cpu().numpy().tobytes()


def test_gpu_checksum_lengths(eng):
    pc.check_checksum_lengths(eng)


def test_gpu_checksum_alignment(eng):
    pc.check_checksum_alignment(eng, _upload, _download, _alloc)


def test_gpu_checksum_uncompress(eng):
    pc.check_checksum_uncompress(eng, _upload, _download, _alloc)


def test_gpu_checksum_piece_counts(eng):
    pc.check_checksum_piece_counts(eng, _upload, _download, _alloc)


def test_gpu_checksum_entry_points(eng):
    pc.check_checksum_entry_points(eng)
