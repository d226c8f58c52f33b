"""Inputs for a BestSpeed matcher that probes ahead (windows of 64 positions on a fixed grid while dense
steps follow each other, the next window's table slots asked for before the walk in front of it has inserted; measured
and not shipped, the kernel is profiles/l1_ahead_attempt.patch).  They hold for any matcher: where a grid would lie
depends on the parse, so every family sweeps its own phase instead of assuming one.  The oracle is the yardstick;
nothing here knows what the kernel does.

    B  one planted repeat: a match of every length class starting at every offset 0 .. 130
    X  two (and three) positions that share a table slot, 1 .. 130 bytes apart: the same four bytes, or other bytes
       with the same 14-bit hash; the earlier one probed, inside a match, or the ip-1 behind a match
    P  short and window-sized periods at every phase
    D  literal runs of 29 .. 40 misses in front of a match from every start 0 .. 63 (the run's 32nd probe switches the
       schedule), and sparse runs that end in a match 1 .. 70 bytes before a multiple of 64
    T  every tail length: the 15-byte rule inside the current and inside the next window
    and a 40 000-byte input whose first fragment ends in a long match

`python tests/l1_ahead_cases.py` checks every input under the emulator.  ZH_L1_AHEAD=0 is the switch that kernel reads
once a process to run without its warm steps: tests/test_emu_l1_ahead.py runs this file as a child once a setting (a
matcher without the switch runs the same code twice)."""
import random
import sys

import numpy as np

HASH_MUL = 0x1E35A7BD
B_LENGTHS = (4, 5, 15, 16, 17, 31, 32, 33, 62, 63, 64, 65, 66, 127, 128, 129, 258, 300)
P_PERIODS = tuple(range(1, 10)) + (31, 32, 33, 63, 64, 65, 127, 128, 129)
D_RUNS = tuple(range(29, 41))
FRAG = 32768


def hash14(four):
    return ((int.from_bytes(four, "little") * HASH_MUL) & 0xFFFFFFFF) >> 18


def dense_filler(rnd, n):
    """n bytes the parse stays dense in: noise with a short repeat of itself every 10 .. 20 bytes, so that no literal
    run comes near its 32nd probe"""
    out = bytearray(rnd.randbytes(min(n, 12)))
    while len(out) < n:
        o = rnd.randrange(0, len(out) - 7)
        out += out[o:o + rnd.randrange(4, 8)]
        out += rnd.randbytes(rnd.randrange(6, 14))
    return bytes(out[:n])


def _other_with_hash(rnd, four):
    """four other bytes with the same 14-bit hash (brute force over the product's top bits)"""
    want = hash14(four)
    while True:
        xs = (np.uint64(rnd.randrange(1 << 16) << 16) + np.arange(1 << 16, dtype=np.uint64))
        hit = np.flatnonzero((((xs * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(18)) == np.uint64(want))
        for i in hit:
            cand = int(xs[i]).to_bytes(4, "little")
            if cand != four:
                assert hash14(cand) == want
                return cand


def _has_match(src, pos, offset):
    import oracle
    import parity_cases as pc
    return any(p == pos and o == offset for p, o, n in pc.token_matches(oracle.block_tokens(src, 1)[0])[0])


def b_cases():
    rnd = random.Random(0xB0)
    out = []
    for length in B_LENGTHS:
        pat = rnd.randbytes(length)
        for s in range(131):
            # the pattern at position 1, filler, the pattern again s bytes later, a byte that ends the match
            brk = bytes([pat[0] ^ 0x55]) if length else b""
            src = b"\x01" + pat + b"\xfe" + dense_filler(rnd, s) + pat + brk + rnd.randbytes(20)
            assert len(src) <= 1024
            out.append(("B/len%d_at%d" % (length, s), src))
    return out


def x_cases():
    """(name, src, (first position, second position) or None)"""
    rnd = random.Random(0xC5)
    out = []
    for d in range(1, 131):
        q = rnd.randbytes(4)
        if d < 4:  # the same four bytes d apart: a period of d
            q = (q[:d] * 4)[:4]
        other = _other_with_hash(rnd, q)
        lead = dense_filler(rnd, 24 + (d * 7) % 64)
        between = dense_filler(rnd, d - 4) if d >= 4 else b""
        long_ = rnd.randbytes(24)  # a repeat that swallows what stands inside it
        for kind, second in (("same", q), ("hash", other)):
            if d < 4 and kind == "hash":
                continue
            # (i) the earlier position is probed in a literal run (these inputs are short and their tables small: the
            # bytes around are drawn again until nothing between the two takes the slot, which the oracle's tokens say)
            for _ in range(200):
                if d >= 4:
                    body = lead + q + between + second
                else:
                    body = lead + (q[:d] * 8)[:d + 4]
                src = b"\x02" + body + rnd.randbytes(24)
                where = (1 + len(lead), 1 + len(lead) + d)
                if kind != "same" or _has_match(src, where[1], d):
                    break
                lead = dense_filler(rnd, len(lead))
                between = dense_filler(rnd, d - 4) if d >= 4 else b""
            out.append(("X/%s_probed_d%d" % (kind, d), src, where if kind == "same" else None))
            if d < 4:
                continue
            # (ii) the earlier position lies inside a match and is never inserted; for "hash" the slot holds an older
            # position with the second one's bytes, which a stale read would turn into a match
            if d >= 20:
                inner = long_[:8] + q + long_[8:]
                src = b"\x03" + inner + second + rnd.randbytes(9) + lead + inner + between[:d - 20] + second + rnd.randbytes(24)
                out.append(("X/%s_inside_d%d" % (kind, d), src, None))
            # (iii) the earlier position is the ip-1 behind a match: the match's last byte starts q
            rep = long_[:9] + q[:1]
            src = b"\x04" + rep + rnd.randbytes(7) + second + rnd.randbytes(5) + lead + rep + q[1:] + between + second + rnd.randbytes(24)
            out.append(("X/%s_behind_d%d" % (kind, d), src, None))
        # three positions in a row with q's slot, of which only the middle one is inserted, and a fourth that asks
        if d >= 12:
            inner = long_[:8] + q + long_[8:20]
            src = (b"\x05" + inner + rnd.randbytes(9) + lead + inner + rnd.randbytes(3) + q + rnd.randbytes(5) + inner +
                   between[:max(0, d - 32)] + q + rnd.randbytes(24))
            out.append(("X/three_d%d" % d, src, None))
    return out


def p_cases():
    rnd = random.Random(0xD7)
    out = []
    for p in P_PERIODS:
        pat = rnd.randbytes(p)
        for phase in range(64):
            src = rnd.randbytes(phase) + pat * (4096 // p + 1)
            out.append(("P/period%d_phase%d" % (p, phase), src[:4096]))
    return out


def d_cases():
    """(name, src, position of the planted match or None)"""
    rnd = random.Random(0xE9)
    out = []
    key = rnd.randbytes(12)
    def planted(src, at, exact):  # the oracle finds the key's repeat (these tables are small: another draw where the slot was taken)
        import oracle
        import parity_cases as pc
        return any(0 <= p - at < (1 if exact else 8) and o == at - 1
                   for p, o, n in pc.token_matches(oracle.block_tokens(src, 1)[0])[0])

    for run in D_RUNS:
        for start in range(64):
            # a short match ends the filler; `run` bytes of noise behind it; then the key, which stands at position 1
            # (drawn again while the oracle does not find the key where it begins: after 40 draws it is the schedule
            # that steps over that byte, not a slot taken by the noise)
            best = None
            for _ in range(40):
                head = b"\x06" + key + b"\xfd" + dense_filler(rnd, 20 + start)
                src = head + head[15:21] + rnd.randbytes(run) + key + rnd.randbytes(24)
                if planted(src, len(head) + 6 + run, True):
                    best = src
                    break
                if best is None and planted(src, len(head) + 6 + run, False):
                    best = src
            src = best
            out.append(("D/run%d_start%d" % (run, start), src, len(head) + 6 + run))
    for back in range(1, 71):
        at = 64 * 6 - back
        for _ in range(200):
            src = b"\x07" + key + rnd.randbytes(at - 13) + key + rnd.randbytes(40)
            if planted(src, at, False):
                break
        out.append(("D/sparse_%d_before_grid" % back, src, at))
    return out


def t_cases(text):
    out = [("T/len%d" % n, text[500:500 + n]) for n in range(301)]
    out += [("T/frag_minus%d" % k, text[1000:1000 + FRAG - k]) for k in range(21)]
    return out


def two_fragments(text):
    chunk = text[2000:2050]
    src = text[3000:3000 + FRAG - 300] + chunk * 14 + text[40000:]
    return [("two_fragments", src[:40000])]


def all_cases():
    """[(name, bytes)]: about 6 000 inputs, under 20 MiB"""
    import synth
    text = synth.corpus_file("alice29.txt")
    cases = b_cases() + [c[:2] for c in x_cases()] + p_cases() + [c[:2] for c in d_cases()] + t_cases(text) + two_fragments(text)
    assert sum(len(c[1]) for c in cases) < 20 << 20
    return cases


def check_emu(stride=1):
    """every case byte-identical to the oracle at level 1 (raw deflate), and the match list of every `stride`-th equal to
    the oracle's tokens; -> (inputs, match lists compared)"""
    import emu
    import oracle
    import parity_cases as pc
    eng = emu.engine()
    cases = all_cases()
    bufs = [c[1] for c in cases]
    outs, sts = eng.compress_batch(bufs, 1, oracle.dfDeflate)
    for (name, src), out, st in zip(cases, outs, sts):
        assert st == 0, (name, st)
        assert out == oracle.deflate(src, 1), name
    compared = 0
    for name, src in cases[::stride]:
        dev = eng.debug_tokens(src, 1)
        assert np.array_equal(dev, oracle.block_tokens(src, 1)[0]), name
        compared += 1
    return len(cases), compared


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("l1_ahead_cases ok: %d inputs, %d match lists" % check_emu(int(sys.argv[1]) if len(sys.argv) > 1 else 1))
