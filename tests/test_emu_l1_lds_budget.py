"""CPU-only: the cases of tests/l1_lds_budget_cases.py under the fiber emulator, one child process a setting.  The
emulator's streams run one after the other, so in the plan of all buffers the pooled waves take every fragment but the
LDS-table waves' first tickets; in the plans of one buffer of P + L fragments the last L are the LDS-table waves'."""
import pytest

import l1_lds_budget_cases as lc


@pytest.mark.parametrize("p,l", lc.SETTINGS)
def test_emu_l1_lds_budget(p, l):
    lc.run_child("emu", p, l, 1800)


def test_cases_are_what_they_claim():
    """every kind of case is there, no buffer is longer than three fragments, buffers of P + L fragments exist for
    every mixed setting, and the crafted groups share what they should: the folded hash but not the bytes, or the bytes"""
    cs = lc.cases()
    names = [n for n, _ in cs]
    assert len(set(names)) == len(names)
    for kind in ("fold", "same"):
        for k in lc.GROUPS:
            assert "flags %s %d" % (kind, k) in names
    assert all("period %d" % p in names for p in lc.PERIODS)
    assert all("alphabet %d" % a in names for a in lc.ALPHABETS)
    for s in lc.FRAG_SIZES:
        assert len(dict(cs)["fragment %d alone" % s]) == s
        assert len(dict(cs)["fragment %d behind a full one" % s]) == lc.FRAG + s
    assert sum(n.startswith("carry") for n in names) == 6
    assert max(len(b) for _, b in cs) == lc.MAX_BUFFER
    nfrags = {(len(b) + lc.FRAG - 1) // lc.FRAG for _, b in cs}
    for p, l in lc.SETTINGS:
        assert 1 <= p <= 3 and l <= 2
        assert not l or any(n >= p + l for n in nfrags) or p + l > 3
    assert {2, 3} <= nfrags
    assert lc.check_flag_buffers() >= 6 * 20
