"""CPU-only: the resumable uncompress (zippy_amd/csrc/zh_resume.hip: zh_uncompress_resume_batch with the resuming form
of the wave-pair inflate, zh_inflate_pair.h) under the fiber emulator of tests/hipemu.  The cases are
tests/resume_cases.py's, shared with tests/test_gpu_resume.py; every expectation is the model's (tests/resume_model.py).
The emulator takes 20 ms a stream: here every prefix of the small stream runs in one container, with `last` on every
fifth, the 1-byte chain and two of the mix chains are left to the GPU, and the hand-built streams are the small set,
a stream with more than twelve cuts resumed at a spread of them (resume_cases.spread); the GPU runs every cut."""
import pytest

import emu
import resume_cases as rc
import resume_model as rm


@pytest.fixture(scope="module")
def eng():
    return emu.engine()


def test_emu_resume_every_cut(eng):
    rc.check_every_cut(eng, (rm.DF_GZIP,), last_stride=5)


def test_emu_resume_chains(eng):
    rc.check_chain_small(eng)
    rc.check_chain_mix(eng, ((70001, rc.BIG),))


def test_emu_resume_budget(eng):
    rc.check_budget(eng)


def test_emu_resume_window_edge(eng):
    rc.check_window_edge(eng)


def test_emu_resume_damage(eng):
    rc.check_trailers(eng)
    rc.check_flips(eng)
    rc.check_static_damage(eng)
    rc.check_batch33(eng)


def test_emu_resume_crafted(eng):
    rc.check_crafted(eng, small_set=True, cap=12)


def test_emu_resume_members_and_call_errors(eng):
    rc.check_members(eng)
    rc.check_call_errors(eng)


def test_emu_resume_scratch_groups(eng, monkeypatch, capfd):
    """a budget of 1 MiB: the streams take the scratch in turns, with the same answers"""
    monkeypatch.setenv("ZH_SCRATCH_MB", "1")
    monkeypatch.setenv("ZH_TRACE", "1")
    z, plain = rc.small(rm.DF_ZLIB)
    want = rc.check(eng, [(None, z, 400000, False)] * 5)
    assert all(w[0] == plain for w in want) and "resume scratch for" in capfd.readouterr().err


def test_emu_resume_api(eng, monkeypatch):
    from zippy_amd import api
    from zippy_amd.common import ZippyError
    monkeypatch.setattr(api, "_engine", eng)
    z, plain = rc.small(rm.DF_GZIP)
    inf = api.Inflater(max_out=256)
    got = b"".join(inf.feed(z[o:o + 500]) for o in range(0, len(z), 500)) + inf.feed(b"more", last=True)
    assert got == plain and inf.done and inf.unused == b"more" and inf.max_out > 256
    assert b"".join(api.uncompress_chunks(z[o:o + 333] for o in range(0, len(z), 333))) == plain
    with pytest.raises(ZippyError):
        list(api.uncompress_chunks([z[:900], z[901:]]))
    with pytest.raises(ZippyError):
        list(api.uncompress_chunks([z[:-3]]))
