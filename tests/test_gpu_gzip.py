"""zh_gzip_read_batch on a real MI355X (-m gpu): any gzip file -- several members, FEXTRA, FNAME, FCOMMENT, FHCRC --
(zippy_amd/csrc/zh_gzip.hip) against tests/gzip_model.py.  The shared cases are tests/gzip_cases.py's, as under the
emulator (tests/test_emu_gzip.py); every one runs as it is and once more with ZH_GZIP_SPEC_BYTES=0, which sizes every
member by frontier rounds."""
import pytest

import gzip_cases as gc

pytestmark = pytest.mark.gpu

BUDGETS = (None, 0)


@pytest.fixture(scope="module")
def eng():
    import torch  # torch's bundled HIP runtime has to initialise before libzippy_hip.so's
    torch.cuda.init()
    from zippy_amd import api
    e = api.engine()
    e.set_gzip_fname_len(0)
    return e


@pytest.mark.parametrize("budget", BUDGETS)
def test_gpu_gzip_chain_lengths(eng, budget):
    gc.check_chain_lengths(eng, budget)


@pytest.mark.parametrize("budget", BUDGETS)
def test_gpu_gzip_33_images(eng, budget):
    gc.check_batch_33(eng, budget)


@pytest.mark.parametrize("budget", BUDGETS)
def test_gpu_gzip_1600_members(eng, budget):
    gc.check_1600_members(eng, budget)


@pytest.mark.parametrize("budget", BUDGETS)
def test_gpu_gzip_fixtures(eng, budget):
    gc.check_fixtures(eng, budget)


@pytest.mark.parametrize("budget", BUDGETS)
def test_gpu_gzip_stream_ends(eng, budget):
    gc.check_stream_ends(eng, budget)


@pytest.mark.parametrize("budget", BUDGETS)
def test_gpu_gzip_header_fields(eng, budget):
    gc.check_header_fields(eng, budget)


@pytest.mark.parametrize("budget", BUDGETS)
def test_gpu_gzip_bgzf_file_as_gzip(eng, budget):
    gc.check_bgzf_as_gzip(eng, budget)


@pytest.mark.parametrize("budget", BUDGETS)
def test_gpu_gzip_false_candidates(eng, budget):
    gc.check_false_candidates(eng, budget)


@pytest.mark.parametrize("budget", BUDGETS)
def test_gpu_gzip_signature_straddling(eng, budget):
    gc.check_straddling(eng, budget)


@pytest.mark.parametrize("budget", BUDGETS)
def test_gpu_gzip_ends(eng, budget):
    gc.check_ends(eng, budget)


def test_gpu_gzip_adversarial_image_under_budget(eng):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    gc.check_adversarial(eng, in_flight=lambda candidates: gc.resident_workgroups(candidates, cus), unbudgeted_run=True)


def test_gpu_gzip_nul_search_under_budget(eng):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # (the header kernel: a wave a candidate, four a workgroup, at most 32 waves a CU)
    gc.check_nul_search_budget(eng, 16383, head_in_flight=lambda candidates: min(candidates, cus * 32),
                               spec_in_flight=lambda candidates: gc.resident_workgroups(candidates, cus))


def test_gpu_gzip_interface(eng):
    gc.check_interface(eng)


def test_gpu_gzip_api(eng):
    from zippy_amd import api
    gc.check_api(eng, api)
