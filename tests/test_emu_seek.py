"""CPU-only: seek indexes for foreign deflate streams (zippy_amd/csrc/zh_seek.hip: zh_seek_index_batch,
zh_seek_read_ranges, with the recording form of zh_inflate_tokens_kernel and the seek form of zh_inflate_kernel) under
the fiber emulator of tests/hipemu.  The cases are tests/seek_cases.py's, shared with tests/test_gpu_seek.py; the
expected blobs are the model's (tests/seek_model.py), the expected bytes slices of the original input.  The emulator
takes a second a 340 KiB stream: the read and damage cases run on one container of the first family here, on all three
on the GPU."""
import pytest

import emu
import seek_cases as sc
import seek_model as sm


@pytest.fixture(scope="module")
def eng():
    return emu.engine()


def test_emu_seek_build_family(eng):
    sc.check_build_family(eng)


def test_emu_seek_build_spans(eng):
    sc.check_build_spans(eng)


def test_emu_seek_build_small_own_and_flushed(eng):
    sc.check_build_small_and_own(eng)


def test_emu_seek_build_crafted(eng):
    sc.check_build_crafted(eng)


def test_emu_seek_build_zeros(eng):
    sc.check_build_zeros(eng)


def test_emu_seek_build_list_retry(eng, monkeypatch, capfd):
    sc.check_build_list_retry(eng, monkeypatch, capfd)


def test_emu_seek_batch_of_33(eng):
    sc.check_read_batch33(eng, sc.check_build_batch33(eng))


def test_emu_seek_read_family(eng):
    sc.check_read_family(eng, sc.WBITS[1:2])


def test_emu_seek_upload_accounting(eng):
    sc.check_upload_accounting(eng)


def test_emu_seek_scratch_groups(eng, monkeypatch, capfd):
    sc.check_scratch_groups(eng, monkeypatch, capfd)


def test_emu_seek_damaged_bytes(eng):
    sc.check_damaged_bytes(eng, sc.family(-15)[1], sm.DF_DEFLATE)


def test_emu_seek_damaged_window_and_point(eng):
    sc.check_damaged_window(eng)
    sc.check_moved_point(eng)


def test_emu_seek_static_damage_and_call_errors(eng):
    sc.check_static_damage(eng)
    sc.check_call_errors(eng)


def test_emu_seek_api(eng, monkeypatch):
    """api.seek_index / seek_read_range raise; the batch forms hand the statuses out"""
    from zippy_amd import api
    from zippy_amd.common import ZippyError
    monkeypatch.setattr(api, "_engine", eng)
    data = sc.family(31)[0]
    blob = api.seek_index(data, span=sc.SPAN)
    assert blob == sc.model(data, sm.DF_GZIP)[0]
    assert api.seek_read_range(data, blob, 70000, 100) == sc.mix()[70000:70100]
    assert api.seek_read_range(data, blob, len(sc.mix()) + 1, 100) == b""
    with pytest.raises(ZippyError):
        api.seek_index(data[:1000])
    with pytest.raises(ZippyError):
        api.seek_read_range(data, blob[:-1], 0, 10)
    blobs, sts = api.seek_index_batch([data, data[:1000]], span=sc.SPAN)
    assert sts[0] == 0 and sts[1] != 0 and blobs == [blob, None]
    outs, sts = api.seek_read_ranges([data], [blob], [(0, 5, 10)])
    assert (outs, sts) == ([sc.mix()[5:15]], [0])


# ---- points at any block boundary (histories of any length), the hand-built streams, forged windows ----
def test_emu_seek_dense_point_sets(eng):
    sc.check_dense(eng, small=True)


def test_emu_seek_crafted_streams_build(eng):
    sc.check_crafted_all(eng, small=True)


def test_emu_seek_crafted_behind_history(eng):
    sc.check_crafted_behind_history(eng, small=True)


def test_emu_seek_window_edge(eng):
    sc.check_window_edge(eng)


def test_emu_seek_short_interval(eng):
    sc.check_short_interval(eng)
