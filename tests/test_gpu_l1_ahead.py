"""The BestSpeed matcher on the GPU over every input of l1_ahead_cases in ONE batch -- thousands of waves in dense and
sparse steps side by side, the walk's hop loop in its machine-code form -- byte-identical to the oracle, and a batch
of G-mix."""
import numpy as np
import pytest

import l1_ahead_cases as lc
import oracle
import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch  # torch's bundled HIP runtime has to initialise before libzippy_hip.so's
    torch.cuda.init()
    from zippy_amd import api
    e = api.engine()
    e.set_gzip_fname_len(0)
    return e


def test_gpu_l1_ahead_families(eng):
    cases = lc.all_cases()
    bufs = [c[1] for c in cases]
    assert 5000 <= len(bufs) <= 7000 and sum(len(b) for b in bufs) < 20 << 20
    outs, sts = eng.compress_batch(bufs, 1, oracle.dfGzip)
    assert all(s == 0 for s in sts)
    bad = [name for (name, src), out in zip(cases, outs) if out != oracle.compress(src, 1, oracle.dfGzip, fname_len=0)]
    assert not bad, (len(bad), bad[:10])
    step = len(cases) // 64
    for name, src in cases[step // 2::step][:64]:  # a sample across all families
        assert np.array_equal(eng.debug_tokens(src, 1), oracle.block_tokens(src, 1)[0]), name


def test_gpu_l1_ahead_mix(eng):
    bufs = [b.tobytes() for b in synth.gen_batch("mix", 64, 65536, first_index=4242)]
    outs, sts = eng.compress_batch(bufs, 1, oracle.dfGzip)
    assert all(s == 0 for s in sts)
    for i, (src, out) in enumerate(zip(bufs, outs)):
        assert out == oracle.compress(src, 1, oracle.dfGzip, fname_len=0), i
