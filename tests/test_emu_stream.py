"""CPU-only: the streaming compress (zippy_amd/csrc/zh_stream.hip: zh_compress_stream_batch with zh_stream_consts_kernel
and zh_stream_splice_kernel) under the fiber emulator of tests/hipemu.  The cases are tests/stream_cases.py's, shared
with tests/test_gpu_stream.py; every expectation is the model's (tests/stream_model.py).
Thinned for the emulator's speed, the GPU runs the rest: the alignment family is the covering few of
stream_cases.align_cover() with the formats taking turns (the model asserts that they reach every k, both byte deltas,
every (p + 3) mod 8, every pending count and every marker residue); the length x level grid runs levels 1, 0 and 6 in
one format each.  The stored and empty families, the identity and the rest run whole."""
import pytest

import emu
import stream_cases as sc
import stream_model as sm


@pytest.fixture(scope="module")
def eng():
    return emu.engine()


def test_emu_stream_alignment(eng):
    sc.check_align(eng, thin=True)


@pytest.mark.parametrize("level,fmt", ((1, sm.DF_GZIP), (0, sm.DF_ZLIB), (6, sm.DF_DEFLATE)))
def test_emu_stream_lengths(eng, level, fmt):
    sc.check_lengths(eng, (level,), (fmt,))


def test_emu_stream_stored(eng):
    sc.check_stored(eng)


def test_emu_stream_empty(eng):
    sc.check_empty(eng)


def test_emu_stream_identity(eng):
    sc.check_identity(eng)


def test_emu_stream_batch33_in_scratch_groups(eng, monkeypatch, capfd):
    """a budget of 1 MiB: the streams take the scratch in turns, with the same answers"""
    monkeypatch.setenv("ZH_SCRATCH_MB", "1")
    monkeypatch.setenv("ZH_TRACE", "1")
    sc.check_batch33(eng)
    assert "stream scratch for" in capfd.readouterr().err


def test_emu_stream_bad_states_and_call_errors(eng):
    sc.check_bad_states(eng)
    sc.check_call_errors(eng)


def test_emu_stream_contract_mode(eng):
    sc.check_contract_mode(eng)


def test_emu_stream_fname(eng):
    """the header is zh_compress's: the name zh_set_gzip_fname_len asks for"""
    eng.set_gzip_fname_len(5)
    try:
        sc.check_chains(eng, [sc.Chain([sc.short(40), sc.text(900, 1)], [sc.BLOCK, sc.FINISH], 1, sm.DF_GZIP)], fname_len=5)
    finally:
        eng.set_gzip_fname_len(0)


def test_emu_stream_api(eng, monkeypatch):
    from zippy_amd import api
    monkeypatch.setattr(api, "_engine", eng)
    data = sc.text(40000, 1) + sc.rnd(3000, 1) + sc.text(30000, 2)
    d, inf = api.Deflater(api.BestSpeed, api.dfGzip, 32768), api.Inflater()
    got = b""
    for at in range(0, len(data), 9000):
        got += inf.feed(d.feed(data[at:at + 9000]))
        assert got == data[:at + 9000]  # a sync flush: all that was fed is there
    got += inf.feed(d.finish(), last=True)
    assert got == data and inf.done and d.done and inf.unused == b""
    with pytest.raises(ValueError):
        d.feed(b"more")
    pieces = [data[at:at + 7001] for at in range(0, len(data), 7001)]
    assert b"".join(api.uncompress_chunks(api.compress_chunks(pieces, api.BestSpeed, api.dfZlib, 32768))) == data
    assert api.uncompress(b"".join(api.compress_chunks([], dataFormat=api.dfGzip))) == b""
    z = b"".join(api.compress_chunks([data[:65536], data[65536:]], api.BestSpeed, api.dfGzip, 32768, api.FLUSH_BLOCK))
    assert z == api.compress_blocks(data, api.BestSpeed, api.dfGzip, 32768)[0]
