"""On the MI355X: zh_compress_stream_batch (zippy_amd/csrc/zh_stream.hip).  The cases are tests/stream_cases.py's,
shared with tests/test_emu_stream.py; every expectation -- output, new state, status -- is the model's
(tests/stream_model.py), byte for byte, in all three formats.  Here the alignment family and the length x level grid run
whole, and the default block size is held against the oracle's own compress()."""
import pytest

import stream_cases as sc
import stream_model as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from zippy_amd import api
    e = api.engine()
    e.set_gzip_fname_len(0)
    return e


@pytest.mark.parametrize("fmt", sc.FORMATS)
def test_gpu_stream_alignment(eng, fmt):
    sc.check_align(eng, (fmt,))


@pytest.mark.parametrize("level", sc.LEVELS)
def test_gpu_stream_lengths(eng, level):
    sc.check_lengths(eng, (level,))


def test_gpu_stream_stored(eng):
    sc.check_stored(eng)


def test_gpu_stream_empty(eng):
    sc.check_empty(eng)


def test_gpu_stream_identity(eng):
    sc.check_identity(eng)


def test_gpu_stream_default_block_is_the_reference(eng):
    sc.check_default_block(eng)


def test_gpu_stream_batch33_in_scratch_groups(eng, monkeypatch, capfd):
    """a budget of 1 MiB: the streams take the scratch in turns, with the same answers"""
    monkeypatch.setenv("ZH_SCRATCH_MB", "1")
    monkeypatch.setenv("ZH_TRACE", "1")
    sc.check_batch33(eng)
    assert "stream scratch for" in capfd.readouterr().err


def test_gpu_stream_bad_states_and_call_errors(eng):
    sc.check_bad_states(eng)
    sc.check_call_errors(eng)


def test_gpu_stream_contract_mode(eng):
    sc.check_contract_mode(eng)


def test_gpu_stream_fname(eng):
    eng.set_gzip_fname_len(5)
    try:
        sc.check_chains(eng, [sc.Chain([sc.short(40), sc.text(900, 1)], [sc.BLOCK, sc.FINISH], 1, sm.DF_GZIP)], fname_len=5)
    finally:
        eng.set_gzip_fname_len(0)


def test_gpu_stream_api(eng):
    from zippy_amd import api
    data = sc.text(400000, 1) + sc.rnd(30000, 1) + sc.text(300000, 2)
    d, inf = api.Deflater(api.BestSpeed, api.dfGzip), api.Inflater()
    got = b""
    for at in range(0, len(data), 90000):
        got += inf.feed(d.feed(data[at:at + 90000]))
        assert got == data[:at + 90000]  # a sync flush: all that was fed is there
    got += inf.feed(d.finish(), last=True)
    assert got == data and inf.done and d.done and inf.unused == b""
    pieces = [data[at:at + 70001] for at in range(0, len(data), 70001)]
    assert b"".join(api.uncompress_chunks(api.compress_chunks(pieces, api.DefaultCompression, api.dfZlib))) == data
    z = b"".join(api.compress_chunks([data[:65536], data[65536:]], api.BestSpeed, api.dfGzip, 32768, api.FLUSH_BLOCK))
    assert z == api.compress_blocks(data, api.BestSpeed, api.dfGzip, 32768)[0]
