"""CPU only, no engine: family P (parity_cases.l1p_crafted_inputs) against the mutants of tests/l1p_model.py.  Every
(case, mutant) pair a case declares changes the model's tokens; the declared pairs together are exactly the mutants
that tokens can tell from the rule; no mutant of the other list changes any case; and what each case claims to reach
-- the edges of the rule, and the situations the kernel's speculation has to get right -- is read off the model.
The device runs of the same inputs are in test_emu_parity.py and test_gpu_parity.py (check_l1p_tokens)."""
import pytest

import l1p_model as lm
import parity_cases as pc

CASES = pc.l1p_crafted_inputs()
IDS = [c[0] for c in CASES]
BY_NAME = {c[0]: c for c in CASES}
INFO = pc.l1p_case_info


def base(name):
    return pc.l1p_model_of(name, BY_NAME[name][1])


def lengths(name):
    """the length at EVERY position of a one-fragment case"""
    src = BY_NAME[name][1]
    assert len(src) <= lm.FRAG
    return lm.fragment(src, 0, len(src), [None] * 16384, every=True)


def walk(lens, p, end):
    """the positions a greedy walk from p comes by in front of `end`, and where it leaves"""
    seen = []
    while p < end:
        seen.append(p)
        p += lens[p] or 1
    return seen, p


def chunk_entries(name):
    """[(first position of the chunk, where the parse enters it)] for the kernel's 32-position chunks"""
    starts = [0] + [p + m for p, _, m in base(name)]
    lens = lengths(name)
    _, end = walk(lens, 0, len(lens))
    assert end == len(lens)
    visited = set(walk(lens, 0, len(lens))[0])
    out = []
    for lo in range(0, len(lens), pc.L1P_CHUNK):
        entry = next((p for p in range(lo, len(lens)) if p in visited), None)
        if entry is not None and entry < lo + 258 + pc.L1P_CHUNK:
            out.append((lo, entry))
    assert set(starts) <= visited | {len(lens)}
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_declared_mutants_change_the_tokens(case):
    name, src, kills = case
    for mutant in sorted(kills):
        assert mutant in lm.MUTANTS, (name, mutant)
        assert lm.model(src, mutant) != base(name), "%s: mutant %s gives the rule's tokens" % (name, mutant)


def test_kill_matrix_is_complete():
    declared = set()
    for _, _, kills in CASES:
        declared |= kills
    assert declared == set(lm.MUTANTS)
    assert not set(lm.MUTANTS) & set(lm.INEXPRESSIBLE)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_inexpressible_mutants_change_nothing(case):
    name, src, _ = case
    for mutant in lm.INEXPRESSIBLE:
        assert lm.model(src, mutant) == base(name), "%s: mutant %s can be told from the rule: move it to MUTANTS" % (name, mutant)


def test_inexpressible_mutants_on_the_other_inputs():
    for name, src in pc.l1p_token_cases(small=True):
        if not name.startswith("P/") and len(src) <= 70000:
            for mutant in lm.INEXPRESSIBLE:
                assert lm.model(src, mutant) == pc.l1p_model_of(name, src), (name, mutant)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_covers_the_input(case):
    name, src, _ = case
    got = base(name)
    assert lm.literals(src, got) + sum(m for _, _, m in got) == len(src)
    for mutant in lm.MUTANTS:   # the mutants are parsers too -- but for the two that copy what is not there
        if mutant not in ("lim259", "lim_past_frag"):
            other = lm.model(src, mutant)
            assert lm.literals(src, other) + sum(m for _, _, m in other) == len(src), (name, mutant)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cases_reach_what_they_claim(case):
    name, src, _ = case
    info, got = INFO[name], base(name)
    for m in info.get("has", ()):
        assert m in got, (name, m, got[:3], got[-3:])
    if "none_from" in info:
        assert not [m for m in got if m[0] >= info["none_from"]], (name, got[-2:])
    for p in info.get("none_at", ()):
        assert not [m for m in got if m[0] == p], (name, p)
    for e in info.get("ends_at", ()):
        assert [m for m in got if m[0] + m[2] == e], (name, e)
    if "period" in info:
        period = info["period"]
        assert all(m[1] == period for m in got), name
        for frag_start, n in lm.fragments(len(src)):
            mine = [m for m in got if frag_start <= m[0] < frag_start + n]
            assert mine[0][0] == frag_start + max(period + 1, 2), (name, mine[:2])
            assert all(m[2] == 258 for m in mine[:-1]) and mine[-1][0] + mine[-1][2] >= frag_start + n - 16, (name, mine[-2:])
            # (back to back, but for a literal where the parse lands on a word whose slot another word of the period holds)
            assert all(b[0] - a[0] - a[2] <= 3 for a, b in zip(mine, mine[1:])), name
    if "back_to_back" in info:
        size = info["back_to_back"]
        good = sum(a[2] == size and b[0] == a[0] + size for a, b in zip(got, got[1:]))
        assert good >= 0.8 * len(got) and len(got) >= 0.9 * (len(src) - 37 * size) / size, (name, good, len(got))


def test_fragment_lengths():
    assert [len(BY_NAME["P/len/%d" % n][1]) for n in pc.L1P_TAIL_LENGTHS] == list(pc.L1P_TAIL_LENGTHS)
    assert set(pc.L1P_TAIL_LENGTHS) == {15, 16, 17, 19, 20, 63, 64, 65, 32767, 32768, 32768 + 15, 32768 + 16, 32768 + 19}
    assert base("P/len/15") == base("P/len/16") == base("P/len/17") == []
    # a last fragment of 15 or 16 bytes finds nothing, one of 19 bytes its run
    assert base("P/len/32783")[-1][0] < 32768 - 15 and base("P/len/32784")[-1][0] < 32768 - 15
    assert base("P/len/32787")[-1] == (32768 + 2, 1, 17)


def test_tail_cases_stand_at_the_edge():
    for name, back in (("P/tail/repeat_at_n-16", 16), ("P/tail/repeat_at_n-15", 15)):
        src = BY_NAME[name][1]
        assert src[100:100 + back] == src[-back:] and src[99] != src[-back - 1], name
    assert base("P/tail/repeat_at_n-16")[-1][0] == len(BY_NAME["P/tail/repeat_at_n-16"][1]) - 16
    assert base("P/tail/repeat_at_n-15") == []


def test_zeros_end_with_their_fragment():
    """the kernel's compare runs on into zeroed slack behind the fragment: the rule clips at the fragment's end"""
    for name in ("P/zeros/up_to_fragment_end", "P/zeros/across_fragment_end", "P/zeros/two_fragments_and_19"):
        src = BY_NAME[name][1]
        assert src[pc.FRAG - 500:pc.FRAG] == bytes(500)
        last = [m for m in base(name) if m[0] < pc.FRAG][-1]
        assert last[1] == 1 and last[0] + last[2] == pc.FRAG, (name, last)


def test_back_to_back_matches_defeat_the_guessed_entries():
    """matches of 31 and 33 bytes back to back: the parse enters almost no 32-position chunk at its first byte, and
    where it enters moves by one position a chunk"""
    for size in (31, 33):
        entries = chunk_entries("P/spec/back_to_back_%d" % size)[40:]
        assert len(entries) > 900
        assert sum(entry != lo for lo, entry in entries) >= 0.9 * len(entries), size
        drift = [(b[1] - b[0]) - (a[1] - a[0]) for a, b in zip(entries, entries[1:])]
        assert sum(d in (1, -1) for d in drift) >= 0.8 * len(drift), size
    # 258 and 259: the same over the whole fragment, a match every eight chunks
    for name in ("P/period/258_two_fragments", "P/period/259_two_fragments"):
        got = [m for m in base(name) if m[0] < pc.FRAG]
        assert len(got) >= 126 and sum(m[2] == 258 for m in got) >= len(got) - 1


def test_matches_end_on_chunk_and_wave_edges():
    m = INFO["P/spec/ends_on_chunk_edge"]["has"][0]
    assert (m[0] + m[2]) % pc.L1P_CHUNK == 0 and (m[0] + m[2]) % pc.L1P_WAVE != 0 and m[0] % pc.L1P_CHUNK
    m = INFO["P/spec/ends_on_wave_edge"]["has"][0]
    assert (m[0] + m[2]) % pc.L1P_WAVE == 0 and m[0] // pc.L1P_CHUNK != (m[0] + m[2]) // pc.L1P_CHUNK
    for name in ("P/spec/ends_on_chunk_edge", "P/spec/ends_on_wave_edge"):
        assert len(base(name)) == 1   # (... and the byte behind the edge starts nothing)
    # the periods and the strings of 32 put matches on many more
    assert sum((p + m) % pc.L1P_CHUNK == 0 for p, _, m in base("P/spec/back_to_back_32")) > 500


def test_phase_pair():
    """two inputs that differ only inside their first 20 bytes, whose parses never meet again: the exact entry of the
    first chunk has to be handed through all 1024 chunks and 16 waves before the last tokens are right"""
    a, b = BY_NAME["P/spec/phase_a"][1], BY_NAME["P/spec/phase_b"][1]
    assert len(a) == len(b) == pc.FRAG and a[20:] == b[20:] and a[:20] != b[:20]
    ma, mb = base("P/spec/phase_a"), base("P/spec/phase_b")
    assert (ma[-1][0] - mb[-1][0]) % 33 != 0 and ma[-1][0] > pc.FRAG - 300 and mb[-1][0] > pc.FRAG - 300
    assert not {m[0] for m in ma} & {m[0] for m in mb}
    assert all(b2[0] == a2[0] + a2[2] for ms in (ma, mb) for a2, b2 in zip(ms, ms[1:]))   # one chain of matches each
    for ms in (ma, mb):   # every wave and most chunks lie inside the chain: none can know its entry by itself
        assert {m[0] // pc.L1P_WAVE for m in ms} == set(range(16))
    la, lb = lengths("P/spec/phase_a"), lengths("P/spec/phase_b")
    assert la[300:pc.FRAG - 300] == lb[300:pc.FRAG - 300] and min(la[300:pc.FRAG - 300]) == 258


def test_a_second_walk_meets_known_positions():
    """text: in some chunk the walk from the guessed entry (the chunk's first byte) and the walk from the true entry are
    different walks that share positions -- a thread that walks its chunk again looks those lengths up"""
    name = "P/text/one_fragment"
    lens = lengths(name)
    shared = differ = 0
    for lo, entry in chunk_entries(name):
        hi = min(lo + pc.L1P_CHUNK, len(lens))
        if entry != lo and entry < hi:
            first, final = walk(lens, lo, hi)[0], walk(lens, entry, hi)[0]
            differ += 1
            shared += bool(set(first) & set(final)) and first != final
    assert differ > 300 and shared > 100, (differ, shared)


def test_dense_case_is_near_the_record_limit():
    src = BY_NAME["P/dense/four_byte_matches"][1]
    words = [src[i:i + 4] for i in range(0, 4 * 97 * 2, 4)]
    assert len({w[0] for w in words}) == len({pc.l1p_hash(w) >> 18 for w in words}) == pc.L1P_DENSE_WORDS
    pairs = [src[i:i + 8] for i in range(0, len(src) - 8, 4)]
    assert len(set(pairs)) == len(pairs)
    got = base("P/dense/four_byte_matches")
    assert 7500 < len(got) < 8192   # ZH_MAX_MATCHES_PER_FRAG
    # (four bytes each: a neighbour never repeats -- but for the few that begin on a string's last byte, where the
    # string's own slot was taken)
    assert sum(m[2] == 4 for m in got) >= 0.99 * len(got) and max(m[2] for m in got) <= 8


def test_same_step_case():
    src = BY_NAME["P/same-step/three_in_64_127"][1]
    assert src[70:78] == src[90:98] == src[110:118] and 64 <= 70 and 118 <= 128
    assert base("P/same-step/three_in_64_127") == [(90, 20, 8), (110, 20, 8)]
    assert lm.model(src, "step_granular") == []
    assert "P/same-step/three_in_64_127" in pc.l1p_same_step_cases([(n, s) for n, s, _ in CASES if len(s) < 1000])


def test_two_fragments_case():
    src = BY_NAME["P/two-frags/table_of_fragment_0"][1]
    f = pc.FRAG
    assert src[300:316] == src[f + 100:f + 116] == src[f + 400:f + 416]
    assert (f + 400, 300, 16) in base("P/two-frags/table_of_fragment_0")
    assert not [m for m in lm.model(src, "table_survives") if f + 395 <= m[0] <= f + 412]
    assert len(pc.l1p_multi_fragment_cases()) >= 10
    assert {"P/two-frags/table_of_fragment_0", "P/text/three_fragments", "P/text/40001"} <= {n for n, _ in pc.l1p_multi_fragment_cases()}


def test_every_one_of_an_ordered_pair_once():
    for k in (5, 37, 97):
        seq = pc.every_pair_once(k)
        pairs = list(zip(seq, seq[1:]))
        assert len(pairs) == len(set(pairs)) == k * (k - 1) and all(a != b for a, b in pairs)


def test_sizes():
    assert max(len(c[1]) for c in CASES) <= 3 * pc.FRAG
    assert sum(len(c[1]) for c in CASES) < 1 << 20
    assert sum(len(c[1]) <= 1024 for c in CASES) >= 15
