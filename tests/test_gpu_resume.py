"""On the MI355X: zh_uncompress_resume_batch (zippy_amd/csrc/zh_resume.hip).  The cases are tests/resume_cases.py's,
shared with tests/test_emu_resume.py; every expectation -- output, consumed, why, status and the state byte for byte --
is the model's (tests/resume_model.py)."""
import pytest

import resume_cases as rc
import resume_model as rm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from zippy_amd import api
    return api.engine()


@pytest.mark.parametrize("fmt", rc.FORMATS)
def test_gpu_resume_every_cut(eng, fmt):
    rc.check_every_cut(eng, (fmt,))


def test_gpu_resume_chains_small(eng):
    rc.check_chain_small(eng, (1, 61))


@pytest.mark.parametrize("config", ((4099, 50000), (70001, rc.BIG), (4099, rc.BIG), (70001, 50000)))
def test_gpu_resume_chain_mix(eng, config):
    rc.check_chain_mix(eng, (config,))


def test_gpu_resume_budget(eng):
    rc.check_budget(eng)


def test_gpu_resume_window_edge(eng):
    rc.check_window_edge(eng)


def test_gpu_resume_damage(eng):
    rc.check_trailers(eng)
    rc.check_flips(eng)
    rc.check_static_damage(eng)
    rc.check_batch33(eng)


def test_gpu_resume_crafted(eng):
    rc.check_crafted(eng)


def test_gpu_resume_scratch_groups(eng, monkeypatch, capfd):
    """a budget of 1 MiB: the streams take the scratch in turns, windows and all, with the same answers"""
    monkeypatch.setenv("ZH_SCRATCH_MB", "1")
    monkeypatch.setenv("ZH_TRACE", "1")
    z, plain = rc.small(rm.DF_ZLIB)
    (a,) = rc.check(eng, [(None, z[:1500], rc.BIG, False)])
    assert rm.State(a[2]).win_len > 300
    items = [(None, z, 400000, False), (a[2], z[a[1]:], 400000, False)] * 4 + [(a[2], z[a[1]:-40], 300000, True)]
    want = rc.check(eng, items)
    assert [w[3] for w in want[:8]] == [rm.DONE] * 8 and want[8][4] != 0
    assert "resume scratch for" in capfd.readouterr().err


def test_gpu_resume_members_and_call_errors(eng):
    rc.check_members(eng)
    rc.check_call_errors(eng)


def test_gpu_resume_api(eng):
    from zippy_amd import api
    from zippy_amd.common import ZippyError
    z, plain = rc.small(rm.DF_GZIP)
    inf = api.Inflater(max_out=256)
    got = b"".join(inf.feed(z[o:o + 500]) for o in range(0, len(z), 500)) + inf.feed(b"more", last=True)
    assert got == plain and inf.done and inf.unused == b"more"
    assert b"".join(api.uncompress_chunks(z[o:o + 333] for o in range(0, len(z), 333))) == plain
    with pytest.raises(ZippyError):
        list(api.uncompress_chunks([z[:-3]]))
