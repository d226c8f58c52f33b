"""BGZF on a real MI355X (-m gpu): zh_bgzf_write_batch, zh_bgzf_read_batch, zh_bgzf_index_batch and zh_bgzf_read_ranges
(zippy_amd/csrc/zh_bgzf.hip) against tests/bgzf_model.py and Python's gzip.  The shared cases are tests/bgzf_cases.py's,
as under the emulator (tests/test_emu_bgzf.py)."""
import pytest

import bgzf_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch  # torch's bundled HIP runtime has to initialise before libzippy_hip.so's
    torch.cuda.init()
    from zippy_amd import api
    e = api.engine()
    e.set_gzip_fname_len(0)
    return e


@pytest.mark.parametrize("b", bc.BLOCKS)
def test_gpu_bgzf_write_matrix(eng, b):
    bc.check_write_matrix(eng, blocks=(b,))


def test_gpu_bgzf_write_33_images(eng):
    bc.check_write_33(eng)


def test_gpu_bgzf_write_every_residue(eng):
    bc.check_write_residues(eng)


def test_gpu_bgzf_write_whole_chunks(eng):
    bc.check_write_whole_chunks(eng)


def test_gpu_bgzf_write_fallback(eng):
    bc.check_fallback(eng)


def test_gpu_bgzf_write_contract_mode(eng):
    bc.check_contract_mode(eng)


def test_gpu_bgzf_write_errors(eng):
    bc.check_write_errors(eng)


def test_gpu_bgzf_read_good_images(eng):
    bc.check_good_images(eng)


def test_gpu_bgzf_read_1600_members(eng):
    bc.check_many_members(eng)


def test_gpu_bgzf_read_bad_images(eng):
    bc.check_bad_images(eng)


def test_gpu_bgzf_read_signature_across_images(eng):
    bc.check_straddling_pair(eng)


def test_gpu_bgzf_range_shapes(eng):
    bc.check_range_shapes(eng)


def test_gpu_bgzf_ranges_of_64k_members(eng):
    bc.check_range_big_members(eng)


def test_gpu_bgzf_range_residues(eng):
    bc.check_range_residues(eng)


def test_gpu_bgzf_random_ranges(eng):
    bc.check_random_ranges(eng)


def test_gpu_bgzf_ranges_of_foreign_members(eng):
    bc.check_ranges_foreign_members(eng)


def test_gpu_bgzf_ranges_damaged_member(eng):
    bc.check_damaged_member(eng)


def test_gpu_bgzf_ranges_unsound_indexes(eng):
    bc.check_unsound_indexes(eng)
    bc.check_range_call_errors(eng)


def test_gpu_bgzf_api(eng):
    from zippy_amd import api
    bc.check_api(eng, api)
