"""CPU-only: the names zh_plan_kernel_times reports for every kind of plan (tests/kernel_times_cases.py), under the
fiber emulator of tests/hipemu."""
import pytest

import emu
import kernel_times_cases as kc


@pytest.fixture(scope="module")
def names():
    return kc.collect(emu.engine())


@pytest.mark.parametrize("case", list(kc.EXPECTED))
def test_emu_kernel_time_names(names, case):
    assert names[case] == kc.EXPECTED[case]
