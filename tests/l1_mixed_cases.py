"""The exact BestSpeed matcher's mixed launch (zh_l1_match.hip: P pooled waves and L LDS-table waves, two kernels on two
streams, share one batch of fragments through one ticket counter), small enough to be deterministic: a wave's first
ticket is its own index -- the pooled waves' 0 .. P-1, the LDS-table waves' P .. P+L-1 --, so with at least P + L
fragments every wave of both kernels parses a fragment whatever the timing, and with P + L - 1 the launch is the
pooled kernel alone.

A setting is (ZH_L1_SLOTS, ZH_L1_LDS_WAVES) = (P, L); both are read once a process, so `python tests/l1_mixed_cases.py
gpu|emu` is run as a child, once a setting (tests/test_gpu_l1_mixed.py, tests/test_emu_l1_mixed.py).  An L-only launch
(P = 0) does not exist: ZH_L1_SLOTS is at least 1.

A plan is ONE buffer of nfrags fragments, nfrags in {P+L-1, P+L, 3(P+L)+1, 64}, the last of them ragged: 1, 14, 15, 16
or 32 767 bytes past a multiple of 32 KiB (2 MiB - 1 at most); G-mix or html; level 1 or -2, gzip.  It runs three
times: the first run takes the fragments as numbered, the later ones in the order made of the run before -- dearest
first with fewer than 8 (P + L) fragments, cheapest last otherwise; 64 fragments are at least 8 (P + L) in every
setting and the others fewer.  Every run's stream is the oracle's byte for byte, and the match list the oracle's
tokens.  The eight plans of a setting go through the ten (ragged length, kind) pairs in turn, each setting starting
where the one before stopped, so that the three settings cover every pair.

The child runs with ZH_TRACE, under which every launch of the matcher says how many fragments either kind of wave
took: the parent holds that against expected_launches() -- the mixed launch really happened, nothing was parsed twice
or left out, and each wave took its own first ticket at least."""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

SETTINGS = ((1, 1), (2, 2), (3, 1))
RAGGED = (1, 14, 15, 16, 32767)
KINDS = ("mix", "html")
LEVELS = (1, -2)
FRAG = 32768
_TRACE = re.compile(r"exact matcher: (\d+) pooled waves took (\d+) fragments, (\d+) LDS-table waves (\d+), of (\d+)")


def frag_counts(p, l):
    return (p + l - 1, p + l, 3 * (p + l) + 1, 64)


def plans(p, l):
    """[(name, nfrags, level, kind, ragged)] of the setting (p, l)"""
    out = []
    k = 8 * SETTINGS.index((p, l))
    for nfrags in frag_counts(p, l):
        for level in LEVELS:
            ragged, kind = RAGGED[k % 5], KINDS[k % 2]
            out.append(("%d fragments, level %d, %s, %d past" % (nfrags, level, kind, ragged), nfrags, level, kind, ragged))
            k += 1
    return out


def source(nfrags, kind, ragged, index):
    import synth
    n = (nfrags - 1) * FRAG + ragged
    assert 0 < n < 2 << 20
    return synth.gen_batch(kind, 1, n, first_index=7100 + index)[0].tobytes()


def expected_launches(p, l):
    """[(pooled waves, LDS-table waves, nfrags)] in the order the child launches the matcher: a plan's three runs, then
    its debug_tokens call; and the kernel-times plan's one run"""
    def one(nfrags):
        return (p, l, nfrags) if nfrags >= p + l else (min(p, nfrags), 0, nfrags)
    out = []
    for _, nfrags, _, _, _ in plans(p, l):
        out += [one(nfrags)] * 4
    return out + [one(3 * (p + l) + 1)]


def check_trace(p, l, stderr):
    """the child's ZH_TRACE lines against expected_launches(): -> the number of mixed launches"""
    got = [tuple(int(x) for x in m.groups()) for m in _TRACE.finditer(stderr)]
    want = expected_launches(p, l)
    assert len(got) == len(want), (len(got), len(want), stderr[-2000:])
    mixed = 0
    for (gp, took_p, gl, took_l, gn), (wp, wl, wn) in zip(got, want):
        assert (gp, gl, gn) == (wp, wl, wn), ((gp, gl, gn), (wp, wl, wn))
        assert took_p + took_l == gn and took_p >= gp and took_l >= gl, (gp, took_p, gl, took_l, gn)
        mixed += gl > 0
    return mixed


def run_child(which, p, l, timeout):
    """the setting (p, l) in a fresh process (it starts a child; the caller's process goes on) -> the mixed launches"""
    env = dict(os.environ, ZH_L1_SLOTS=str(p), ZH_L1_LDS_WAVES=str(l), ZH_TRACE="1")
    for k in ("ZH_L1_TABLE", "ZH_L1_ORDER", "ZH_L1_PARSE", "ZH_L1_TAIL_ROUNDS", "ZIPPY_HIP_LIB"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "l1_mixed_cases ok: %d plans" % len(plans(p, l)) in r.stdout, r.stdout[-2000:]
    return check_trace(p, l, r.stderr)


def check(eng, p, l, timed):
    """every plan of the setting three times and its match list; then zh_plan_kernel_times of one mixed level-1 run:
    the names kernel_times_cases pins, nothing of the second stream's kernel, and (`timed`: real events) a matcher
    interval that is not zero"""
    import numpy as np
    import kernel_times_cases as kc
    import oracle
    from ranges_cases import DeviceBuf
    for i, (name, nfrags, level, kind, ragged) in enumerate(plans(p, l)):
        src = source(nfrags, kind, ragged, i)
        want = oracle.compress(src, level, oracle.dfGzip, fname_len=0)
        cap = len(src) + len(src) // 8 + 2048
        d_src, d_dst = DeviceBuf(eng, src + b"\0" * 16), DeviceBuf(eng, bytes(cap))
        plan = eng.plan_compress([0], [len(src)], [0], [cap], level, oracle.dfGzip)
        try:
            for run in range(3):
                d_dst.write(b"\xa5" * cap)
                plan.run(d_src.p, d_dst.p)
                (n,), (st,) = plan.results()
                assert st == 0 and n == len(want) and d_dst.read()[:n] == want, (name, run, st, n, len(want))
        finally:
            plan.close()
            d_src.free()
            d_dst.free()
        assert np.array_equal(eng.debug_tokens(src, level), oracle.block_tokens(src, level)[0]), name
    nfrags = 3 * (p + l) + 1
    src = source(nfrags, "mix", 15, 99)
    cap = len(src) + len(src) // 8 + 2048
    d_src, d_dst = DeviceBuf(eng, src + b"\0" * 16), DeviceBuf(eng, bytes(cap))
    plan = eng.plan_compress([0], [len(src)], [0], [cap], 1, oracle.dfGzip)
    try:
        plan.set_profiling(True)
        plan.run(d_src.p, d_dst.p)
        (n,), (st,) = plan.results()
        assert st == 0 and d_dst.read()[:n] == oracle.compress(src, 1, oracle.dfGzip, fname_len=0)
        times = plan.kernel_times()
    finally:
        plan.close()
        d_src.free()
        d_dst.free()
    assert [name for name, _ in times] == kc.EXPECTED["compress level 1 gzip"], times
    if timed:
        assert times[0][1] > 0, times
    return len(plans(p, l))


if __name__ == "__main__":
    sys.path[:0] = [ROOT, HERE]
    P, L = int(os.environ["ZH_L1_SLOTS"]), int(os.environ["ZH_L1_LDS_WAVES"])
    if sys.argv[1] == "gpu":
        import torch  # torch's bundled HIP runtime has to initialise before libzippy_hip.so's
        torch.cuda.init()
        from zippy_amd import api
        engine = api.engine()
        engine.set_gzip_fname_len(0)
    else:
        import emu
        engine = emu.engine()
    print("l1_mixed_cases ok: %d plans" % check(engine, P, L, sys.argv[1] == "gpu"))
