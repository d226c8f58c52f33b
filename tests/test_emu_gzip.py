"""CPU-only: zh_gzip_read_batch (zippy_amd/csrc/zh_gzip.hip: any gzip file -- several members, FEXTRA, FNAME, FCOMMENT,
FHCRC) under the fiber emulator of tests/hipemu, against tests/gzip_model.py.  The cases are tests/gzip_cases.py's,
shared with tests/test_gpu_gzip.py; every one runs as it is and once more with ZH_GZIP_SPEC_BYTES=0, which sizes every
member by frontier rounds."""
import pytest

import emu
import gzip_cases as gc

BUDGETS = (None, 0)


@pytest.fixture(scope="module")
def eng():
    return emu.engine()


@pytest.mark.parametrize("budget", BUDGETS)
def test_emu_gzip_chain_lengths(eng, budget):
    gc.check_chain_lengths(eng, budget)


@pytest.mark.parametrize("budget", BUDGETS)
def test_emu_gzip_33_images(eng, budget):
    gc.check_batch_33(eng, budget)


@pytest.mark.parametrize("budget", BUDGETS)
def test_emu_gzip_1600_members(eng, budget):
    gc.check_1600_members(eng, budget)


@pytest.mark.parametrize("budget", BUDGETS)
def test_emu_gzip_fixtures(eng, budget):
    gc.check_fixtures(eng, budget, list_alone=False)  # (the tarball of 3.9 MB takes the emulator half a minute a decode)


@pytest.mark.parametrize("budget", BUDGETS)
def test_emu_gzip_stream_ends(eng, budget):
    gc.check_stream_ends(eng, budget)


@pytest.mark.parametrize("budget", BUDGETS)
def test_emu_gzip_header_fields(eng, budget):
    gc.check_header_fields(eng, budget)


@pytest.mark.parametrize("budget", BUDGETS)
def test_emu_gzip_bgzf_file_as_gzip(eng, budget):
    gc.check_bgzf_as_gzip(eng, budget)


@pytest.mark.parametrize("budget", BUDGETS)
def test_emu_gzip_false_candidates(eng, budget):
    gc.check_false_candidates(eng, budget)


@pytest.mark.parametrize("budget", BUDGETS)
def test_emu_gzip_signature_straddling(eng, budget):
    gc.check_straddling(eng, budget)


@pytest.mark.parametrize("budget", BUDGETS)
def test_emu_gzip_ends(eng, budget):
    gc.check_ends(eng, budget)


def test_emu_gzip_adversarial_image_under_budget(eng):
    gc.check_adversarial(eng, in_flight=lambda candidates: 1, unbudgeted_run=False)  # (one workgroup runs at a time)


def test_emu_gzip_nul_search_under_budget(eng):
    one = lambda candidates: 1  # (one workgroup runs at a time)
    gc.check_nul_search_budget(eng, 2048, head_in_flight=one, spec_in_flight=one)


def test_emu_gzip_interface(eng):
    gc.check_interface(eng)


def test_emu_gzip_api(eng, monkeypatch):
    from zippy_amd import api
    monkeypatch.setattr(api, "_engine", eng)
    gc.check_api(eng, api)
