"""CPU-only: the cases of tests/l1_mixed_cases.py under the fiber emulator, one child process a setting.  The emulator's
streams run one after the other, so the pooled kernel takes every fragment but the LDS-table waves' first tickets: that
still proves the ticket bases, the counter's start, the join in front of the code builder and the product build's
LDS-table instantiation."""
import pytest

import l1_mixed_cases as mc


@pytest.mark.parametrize("p,l", mc.SETTINGS)
def test_emu_l1_mixed(p, l):
    mixed = mc.run_child("emu", p, l, 1800)
    assert mixed == sum(4 for _, nfrags, _, _, _ in mc.plans(p, l) if nfrags >= p + l) + 1


def test_cases_cross_what_they_claim():
    """every (ragged length, kind) pair, both levels and both ordering branches in every setting; 2 MiB at most"""
    pairs = set()
    for p, l in mc.SETTINGS:
        ps = mc.plans(p, l)
        pairs |= {(ragged, kind) for _, _, _, kind, ragged in ps}
        assert {level for _, _, level, _, _ in ps} == set(mc.LEVELS)
        assert {nfrags for _, nfrags, _, _, _ in ps} == set(mc.frag_counts(p, l))
        grid = p + l
        assert any(grid < nfrags < 8 * grid for nfrags in mc.frag_counts(p, l))   # dearest first
        assert any(nfrags >= 8 * grid for nfrags in mc.frag_counts(p, l))         # cheapest last
        assert max((nfrags - 1) * mc.FRAG + ragged for _, nfrags, _, _, ragged in ps) < 2 << 20
    assert pairs == {(r, k) for r in mc.RAGGED for k in mc.KINDS}
