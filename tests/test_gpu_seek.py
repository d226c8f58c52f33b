"""Seek indexes for foreign deflate streams on a real MI355X (-m gpu): zh_seek_index_batch and zh_seek_read_ranges
(zippy_amd/csrc/zh_seek.hip).  The shared cases are tests/seek_cases.py's, as under the emulator
(tests/test_emu_seek.py); the expected blobs are the model's (tests/seek_model.py), byte for byte."""
import pytest

import seek_cases as sc
import seek_model as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch  # torch's bundled HIP runtime has to initialise before libzippy_hip.so's
    torch.cuda.init()
    from zippy_amd import api
    e = api.engine()
    e.set_gzip_fname_len(0)
    return e


def test_gpu_seek_build_family(eng):
    sc.check_build_family(eng)


def test_gpu_seek_build_spans(eng):
    sc.check_build_spans(eng)


def test_gpu_seek_build_small_own_and_flushed(eng):
    sc.check_build_small_and_own(eng)


def test_gpu_seek_build_crafted(eng):
    sc.check_build_crafted(eng)


def test_gpu_seek_build_zeros(eng):
    sc.check_build_zeros(eng)


def test_gpu_seek_build_list_retry(eng, monkeypatch, capfd):
    sc.check_build_list_retry(eng, monkeypatch, capfd)


def test_gpu_seek_batch_of_33(eng):
    sc.check_read_batch33(eng, sc.check_build_batch33(eng))


def test_gpu_seek_read_family(eng):
    sc.check_read_family(eng)


def test_gpu_seek_upload_accounting(eng):
    sc.check_upload_accounting(eng)


def test_gpu_seek_scratch_groups(eng, monkeypatch, capfd):
    sc.check_scratch_groups(eng, monkeypatch, capfd)


@pytest.mark.parametrize("wbits,fmt", sc.WBITS)
def test_gpu_seek_damaged_bytes(eng, wbits, fmt):
    for j, data in enumerate(sc.family(wbits)):
        sc.check_damaged_bytes(eng, data, fmt, seed0=1 + 100 * j)


def test_gpu_seek_damaged_window_and_point(eng):
    sc.check_damaged_window(eng)
    sc.check_moved_point(eng)


def test_gpu_seek_static_damage_and_call_errors(eng):
    sc.check_static_damage(eng)
    sc.check_call_errors(eng)


# ---- points at any block boundary (histories of any length), the hand-built streams, forged windows ----
def test_gpu_seek_dense_point_sets(eng):
    sc.check_dense(eng)


def test_gpu_seek_crafted_streams_build(eng):
    sc.check_crafted_all(eng)


def test_gpu_seek_crafted_behind_history(eng):
    sc.check_crafted_behind_history(eng)


def test_gpu_seek_window_edge(eng):
    sc.check_window_edge(eng)


def test_gpu_seek_short_interval(eng):
    sc.check_short_interval(eng)


def test_gpu_seek_batch_of_800(eng, monkeypatch):
    """above ZH_INFLATE_WIDE streams the build takes the narrow recording kernels, which the emulator alone ran so far"""
    sc.check_batch800(eng, monkeypatch)
