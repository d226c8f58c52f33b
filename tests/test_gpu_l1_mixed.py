"""-m gpu: the exact BestSpeed matcher's mixed launch in the product library on a real MI355X -- pooled and LDS-table
waves side by side on two streams, one ticket counter --, the cases of tests/l1_mixed_cases.py, one child process a
setting: every run's stream and match list are the oracle's, zh_plan_kernel_times reports the pinned names with a
matcher interval that is not zero, and the launches were the mixed ones wherever there were fragments enough."""
import pytest

import l1_mixed_cases as mc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("p,l", mc.SETTINGS)
def test_gpu_l1_mixed(p, l):
    mixed = mc.run_child("gpu", p, l, 600)
    assert mixed == sum(4 for _, nfrags, _, _, _ in mc.plans(p, l) if nfrags >= p + l) + 1
