"""The BestSpeed matcher under the emulator (no GPU) on the inputs of l1_ahead_cases: every input byte-identical to the
oracle and its match list equal to the oracle's tokens, with ZH_L1_AHEAD unset and with ZH_L1_AHEAD=0 (the switch of
the matcher's probe-ahead form; it is read once a process, so each setting runs in a process of its
own)."""
import os
import subprocess
import sys

import l1_ahead_cases as lc
import oracle
import parity_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))


def _child(setting):
    env = dict(os.environ)
    env.pop("ZH_L1_AHEAD", None)
    if setting is not None:
        env["ZH_L1_AHEAD"] = setting
    r = subprocess.run([sys.executable, os.path.join(HERE, "l1_ahead_cases.py")], env=env, capture_output=True, text=True,
                       timeout=1800)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "l1_ahead_cases ok: " in r.stdout, r.stdout[-2000:]
    n, m = [int(w) for w in r.stdout.split("ok:")[1].replace(",", " ").split() if w.isdigit()]
    assert n == m == len(lc.all_cases())


def test_emu_l1_ahead_cases_default():
    _child(None)


def test_emu_l1_ahead_cases_switched_off():
    _child("0")


def test_generators_reach_their_corners():
    """from the oracle alone: family X's two positions really are a match and its candidate, at every distance 1 .. 130
    (the candidate lies in the 64 positions before, and in the window before that); family D's planted match is found
    where it stands while the run is dense and a byte later once the run's 32nd probe has switched the schedule; the
    sparse runs end in a match at every distance 1 .. 70 before a multiple of 64; the first of the two fragments ends
    in a match"""
    seen = set()
    for name, src, where in lc.x_cases():
        if where is None:
            continue
        matches, covered = pc.token_matches(oracle.block_tokens(src, 1)[0])
        assert covered == len(src)
        first, second = where
        d = second - first
        if any(p == second and o == d for p, o, n in matches):
            seen.add(d)
    assert seen == set(range(1, 131)), sorted(set(range(1, 131)) - seen)
    late, sparse_back = {}, set()
    for name, src, at in lc.d_cases():
        matches, _ = pc.token_matches(oracle.block_tokens(src, 1)[0])
        found = [p - at for p, o, n in matches if 0 <= p - at < 8 and o == at - 1]
        if name.startswith("D/run"):
            assert found, name
            late.setdefault(int(name[5:].split("_")[0]), set()).add(found[0])
        elif found:
            assert (at + int(name.split("_")[1])) % 64 == 0
            sparse_back.add(int(name.split("_")[1]))
    stepped = [run for run in lc.D_RUNS if late[run] != {0}]
    assert stepped and stepped[0] in (32, 33, 34), late        # up to there the key is found where it stands: dense
    # then every second byte is probed: the key is stepped over and found a byte later (where the match in front of
    # the noise ended an odd number of bytes before it), and a run one byte longer is found where it stands again
    assert 1 in late[stepped[0]] and late[stepped[0]] <= {0, 1} and late[stepped[0] + 1] == {0}, late
    assert sparse_back == set(range(1, 71)), sorted(set(range(1, 71)) - sparse_back)
    (_, src), = lc.two_fragments(__import__("synth").corpus_file("alice29.txt"))
    matches, _ = pc.token_matches(oracle.block_tokens(src, 1)[0])
    assert len(src) == 40000 and any(p < lc.FRAG and p + n == lc.FRAG and n >= 100 for p, o, n in matches)
    cases = lc.all_cases()
    assert 5000 <= len(cases) <= 7000 and {c[0].split("/")[0] for c in cases} == {"B", "X", "P", "D", "T", "two_fragments"}
    assert {len(c[1]) for c in cases if c[0].startswith("T/len")} == set(range(301))
