"""The exact BestSpeed matcher's LDS budget (zh_l1_match.hip: step flags `seen` / `dup` in place of byte counters, the
histograms as packed pairs, one 4 KiB region that is the parse's maps first and the coverage bitmap afterwards), for
the emulator and the GPU from one list of cases.

Every buffer is at most 96 KiB = three fragments, so with few waves one wave takes several fragments in a row and
carries its LDS from one to the next.  A setting is (ZH_L1_SLOTS, ZH_L1_LDS_WAVES) = (P, L), read once a process:
`python tests/l1_lds_budget_cases.py gpu|emu` runs as a child, once a setting (tests/test_gpu_l1_lds_budget.py,
tests/test_emu_l1_lds_budget.py).  L = 0 is the pooled kernel alone with one or two waves; the others are the mixed
launch wherever a plan has P + L fragments: a wave's first ticket is its own index, so in a buffer of P + L fragments
the last L are parsed by LDS-table waves whatever the timing.

Per buffer: the stream at level 1 and at level -2 against oracle.compress byte for byte, zh_debug_tokens against
oracle.block_tokens.  Then all buffers as ONE plan at either level, run twice (the second run in the order made of the
first one's costs): some seventy fragments through P + L waves.

The cases:
  flags      4-byte groups found on the CPU with the kernel's hash constant, 2, 3 and 8 of them within 64 positions:
             `fold` -- different bytes, the same low 12 hash bits, the upper two of the 14 taking turns (flagged; from
             the fifth on also a slot shared by different bytes) --, and `same` -- the same four bytes (a shared slot
             whose true candidate is an earlier lane of the step);
  period     1, 2, 3, 5, 63, 64 and 65 bytes;
  alphabet   2, 3 and 4 symbols, skewed: one symbol's count near a fragment's 32 768 in the packed histogram;
  fragment   a last fragment of 14, 15, 16, 64, 65, 8192, 8193, 32 767 and 32 768 bytes, alone and behind a full one;
  carry      a text fragment, random bytes and zeros in every order: what a wave's LDS holds after one kind must not
             show in the next."""
import itertools
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

SETTINGS = ((1, 0), (2, 0), (1, 1), (1, 2), (2, 2), (3, 1))
LEVELS = (1, -2)
FRAG = 32768
HASH_MUL = 0x1E35A7BD  # zh_l1_match.hip kHashMul (snappy.nim:70-71)
SHIFT = 18             # fragments of 16 384 bytes and more: a 14-bit hash
GROUPS = (2, 3, 8)
PERIODS = (1, 2, 3, 5, 63, 64, 65)
ALPHABETS = (2, 3, 4)
FRAG_SIZES = (14, 15, 16, 64, 65, 8192, 8193, 32767, 32768)
MAX_BUFFER = 3 * FRAG


def hash14(v):
    return ((v * HASH_MUL) & 0xFFFFFFFF) >> SHIFT


def _flag_buffer(kind, k, seed):
    """1024 blocks of 64 bytes = 16 words; in each, k words at places of their own hold the group, the others random
    bytes.  fold: k different words with one folded hash (low 12 bits), upper two bits j & 3; same: one word k times."""
    import numpy as np
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64)
    h = ((pool * HASH_MUL) & 0xFFFFFFFF) >> SHIFT
    order = np.argsort(h, kind="stable")
    hs = h[order]
    first = np.searchsorted(hs, np.arange(1 << 14), "left")
    last = np.searchsorted(hs, np.arange(1 << 14), "right")
    words = rng.integers(0, 1 << 32, (2 * FRAG // 64, 16), dtype=np.uint64)
    for b in range(words.shape[0]):
        places = rng.permutation(16)[:k]
        if kind == "same":
            words[b, places] = words[b, places[0]]
            continue
        while True:
            fold = int(rng.integers(0, 1 << 12))
            if all(last[fold | (j << 12)] - first[fold | (j << 12)] >= 2 for j in range(4)):
                break
        for j, pl in enumerate(places):
            full = fold | ((j & 3) << 12)
            words[b, pl] = pool[order[first[full] + j // 4]]  # (j and j + 4: one slot, different bytes)
    return words.astype("<u4").tobytes()


def check_flag_buffers():
    """the crafted buffers are what the docstring says (CPU only): -> the groups looked at"""
    import numpy as np
    seen = 0
    for name, buf in cases():
        if not name.startswith("flags"):
            continue
        _, kind, k = name.split()
        k = int(k)
        assert len(buf) == 2 * FRAG
        w = np.frombuffer(buf, "<u4").reshape(-1, 16)
        for row in w[:: 37]:
            hv = [hash14(int(v)) for v in row]
            if kind == "same":
                vals, counts = np.unique(row, return_counts=True)
                assert counts.max() == k, (name, counts)
            else:
                folds = {}
                for v, x in zip(row, hv):
                    folds.setdefault(x & 4095, []).append((int(v), x))
                big = max(folds.values(), key=len)
                # (a random word of the block may fall into the group by chance: at least k)
                assert len(big) >= k and len({v for v, _ in big}) == len(big), (name, big)
                assert len({x for _, x in big}) == min(k, 4), (name, big)  # the 14-bit hashes differ (k > 4: in turns)
            seen += 1
    return seen


_cases = None


def cases():
    """[(name, bytes)], every buffer MAX_BUFFER at most; built once a process"""
    global _cases
    if _cases is not None:
        return _cases
    import numpy as np
    import synth
    text = synth.corpus_file("alice29.txt")
    rng = np.random.default_rng(0x1D5B)
    out = []
    for kind in ("fold", "same"):
        for k in GROUPS:
            out.append(("flags %s %d" % (kind, k), _flag_buffer(kind, k, 1000 + 10 * k + (kind == "same"))))
    for p in PERIODS:
        unit = rng.integers(0, 256, p, dtype=np.uint8).tobytes()
        out.append(("period %d" % p, (unit * (40000 // p + 1))[:40000]))
    for a in ALPHABETS:
        prob = np.array([0.97] + [0.03 / (a - 1)] * (a - 1))
        out.append(("alphabet %d" % a, rng.choice(np.arange(65, 65 + a, dtype=np.uint8), 70001, p=prob).tobytes()))
    for s in FRAG_SIZES:
        out.append(("fragment %d alone" % s, text[1000:1000 + s]))
        out.append(("fragment %d behind a full one" % s, text[5000:5000 + FRAG + s]))
    parts = {"text": text[20000:20000 + FRAG], "random": rng.integers(0, 256, FRAG, dtype=np.uint8).tobytes(),
             "zeros": bytes(FRAG)}
    for order in itertools.permutations(sorted(parts)):
        out.append(("carry " + " ".join(order), b"".join(parts[x] for x in order)))
    assert all(0 < len(b) <= MAX_BUFFER for _, b in out)
    _cases = out
    return out


def run_child(which, p, l, timeout):
    """the setting (p, l) in a fresh process (it starts a child; the caller's process goes on)"""
    env = dict(os.environ, ZH_L1_SLOTS=str(p), ZH_L1_LDS_WAVES=str(l))
    for k in ("ZH_L1_TABLE", "ZH_L1_ORDER", "ZH_L1_PARSE", "ZH_L1_TAIL_ROUNDS", "ZH_L1_HEAD_START", "ZIPPY_HIP_LIB", "ZH_TRACE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "l1_lds_budget_cases ok: %d buffers" % len(cases()) in r.stdout, r.stdout[-2000:]


def check(eng):
    import numpy as np
    import oracle
    from ranges_cases import DeviceBuf, pack_streams
    cs = cases()
    want = {level: [oracle.compress(b, level, oracle.dfGzip, fname_len=0) for _, b in cs] for level in LEVELS}

    def run_plan(bufs, level, runs):
        """-> the streams of the last run; every run's are compared"""
        img, off, ln = pack_streams(bufs)
        caps = [n + n // 8 + 2048 for n in ln]
        dst_off = [0]
        for cap in caps[:-1]:
            dst_off.append(dst_off[-1] + ((cap + 255) & ~255))
        total = dst_off[-1] + caps[-1]
        d_src, d_dst = DeviceBuf(eng, img), DeviceBuf(eng, bytes(total))
        plan = eng.plan_compress(off, ln, dst_off, caps, level, oracle.dfGzip)
        try:
            for run in range(runs):
                d_dst.write(b"\xa5" * total)
                plan.run(d_src.p, d_dst.p)
                lens, sts = plan.results()
                got = d_dst.read()
                yield [got[o:o + n] if st == 0 else st for o, n, st in zip(dst_off, lens, sts)]
        finally:
            plan.close()
            d_src.free()
            d_dst.free()

    for i, (name, b) in enumerate(cs):
        for level in LEVELS:
            for out in run_plan([b], level, 1):
                assert out[0] == want[level][i], (name, level)
        assert np.array_equal(eng.debug_tokens(b, 1), oracle.block_tokens(b, 1)[0]), name
    # all of them as one plan: the waves take fragment after fragment, of every kind in turn
    for level in LEVELS:
        for run, out in enumerate(run_plan([b for _, b in cs], level, 2)):
            bad = [cs[i][0] for i in range(len(cs)) if out[i] != want[level][i]]
            assert not bad, (level, run, bad)
    return len(cs)


if __name__ == "__main__":
    sys.path[:0] = [ROOT, HERE]
    if sys.argv[1] == "gpu":
        import torch  # torch's bundled HIP runtime has to initialise before libzippy_hip.so's
        torch.cuda.init()
        from zippy_amd import api
        engine = api.engine()
        engine.set_gzip_fname_len(0)
    else:
        import emu
        engine = emu.engine()
    print("l1_lds_budget_cases ok: %d buffers" % check(engine))
