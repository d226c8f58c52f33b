"""-m gpu: the names zh_plan_kernel_times reports for every kind of plan (tests/kernel_times_cases.py), on a real
MI355X: the lists the emulator gives."""
import pytest

import kernel_times_cases as kc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def names():
    import torch  # torch's bundled HIP runtime has to initialise before libzippy_hip.so's
    torch.cuda.init()
    from zippy_amd import api
    eng = api.engine()
    eng.set_gzip_fname_len(0)
    return kc.collect(eng)


@pytest.mark.parametrize("case", list(kc.EXPECTED))
def test_gpu_kernel_time_names(names, case):
    assert names[case] == kc.EXPECTED[case]
