"""-m gpu: the cases of tests/l1_lds_budget_cases.py in the product library on a real MI355X, one child process a
setting: one or two pooled waves alone, and one to three pooled waves beside one or two LDS-table waves -- every
stream and every match list the oracle's."""
import pytest

import l1_lds_budget_cases as lc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("p,l", lc.SETTINGS)
def test_gpu_l1_lds_budget(p, l):
    lc.run_child("gpu", p, l, 600)
