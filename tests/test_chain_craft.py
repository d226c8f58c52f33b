"""CPU only: family C (parity_cases.chain_crafted_inputs) against the oracle and against the mutants of
tests/chain_model.py.  The model equals the oracle's tokens on every case at every level the case names; every
(level, mutant) pair a case declares changes the tokens of that case; the declared pairs together are the whole kill
matrix; and what each cell claims to reach is read off the model's statistics, the oracle's tokens and numpy.  The
device runs of the same inputs are in test_emu_parity.py and test_gpu_parity.py."""
import numpy as np
import pytest

import chain_model as cm
import oracle
import parity_cases as pc

LEVELS = (2, 3, 4, 5, 6, 7, 8, 9)
# pairs no input can kill (the arguments: chain_model.py's docstring, _c_good_cases and _c_nice_cases)
# (level 9 has no `config+1` at all: the table ends there)
INEXPRESSIBLE = {(lv, "tag4") for lv in (5, 6, 7, 8, 9)} | {(8, "nice_gt"), (9, "nice_gt")} | {(2, "cut_always")}

_memo = {}


def blocks_of(src, size=pc.FULL_BLOCK):
    return [(o, min(size, len(src) - o)) for o in range(0, max(len(src), 1), size)]


def oracle_matches(src, level, start, length):
    return pc.token_matches(oracle.block_tokens(src, level, start, length)[0])[0]


def run(name, src, level):
    """-> (the model's matches of the first block, its statistics by position); the model is held against the
    oracle on every block on the way"""
    key = (name, level)
    if key not in _memo:
        first = None
        for start, length in blocks_of(src):
            stats = []
            got = cm.model(src, level, start, length, stats=stats)
            assert got == oracle_matches(src, level, start, length), (name, level, start)
            if first is None:
                first = (got, {s[0]: s for s in stats})
        _memo[key] = first
    return _memo[key]


CASES = pc.chain_crafted_inputs()
IDS = [c[0] for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_equals_oracle_and_kills(case):
    name, src, levels, kills = case
    assert {lv for lv, _ in kills} <= set(levels), name
    for level in levels:
        got, _ = run(name, src, level)
        for lv, mutant in sorted(kills):
            if lv == level:
                assert cm.has_mutant(level, mutant), (name, level, mutant)
                sizes = pc.CHAIN_BLOCK_SIZES[:1] if name.startswith("C/block/") else (pc.FULL_BLOCK,)
                differs = any(cm.model(src, level, start, length, mutant=mutant, block_size=size) !=
                              oracle_matches(src, level, start, length)
                              for size in sizes for start, length in blocks_of(src, size))
                assert differs, "%s: level %d, mutant %s gives the oracle's tokens" % (name, level, mutant)


def test_kill_matrix_is_complete():
    declared = set()
    for _, _, levels, kills in CASES:
        declared |= {(6 if lv == -1 else lv, m) for lv, m in kills}
        if 6 in levels:   # -1 wherever 6 appears
            assert -1 in levels
            assert {m for lv, m in kills if lv == 6} == {m for lv, m in kills if lv == -1}
    want = {(lv, m) for lv in LEVELS for m in cm.MUTANTS if cm.has_mutant(lv, m)}
    assert INEXPRESSIBLE <= want and (9, "config+1") not in want and len(want) == 8 * len(cm.MUTANTS) - 1
    assert want - declared == INEXPRESSIBLE, sorted(want - declared ^ INEXPRESSIBLE)
    assert not declared & INEXPRESSIBLE


def test_tag4_is_no_mutant_where_records_are_narrow():
    """The premise of the narrow link records (zh_chain_match.hip, "NARROW link records"): at levels 5..9 and -1 a
    candidate that matches fewer than five bytes may count as matching none.  At levels 2..4 it may not."""
    for name, src, levels, kills in CASES:
        for level in levels:
            if level in (2, 3, 4):
                continue
            for start, length in blocks_of(src):
                assert cm.model(src, level, start, length, mutant="tag4") == oracle_matches(src, level, start, length), (name, level)
    assert {lv for c in CASES for lv, m in c[3] if m == "tag4"} == {2, 3, 4}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cells_reach_what_they_claim(case):
    name, src, levels, _ = case
    info = pc.chain_case_info.get(name, {})
    for level in levels:
        got, stats = run(name, src, level)
        if "searcher" in info:
            pos, tried, why, longest, cuts = stats[info["searcher"]]
            if "tried" in info:
                assert tried == info["tried"], (name, level, tried)
            if info.get("why"):
                assert why == info["why"], (name, level, why)
            if "longest" in info:
                assert longest == info["longest"], (name, level, longest)
            if "cuts" in info:
                assert cuts == info["cuts"], (name, level, cuts)
        if "match" in info:
            if info["match"] is None:
                assert not [m for m in got if m[0] == info["searcher"]], (name, level)
            else:
                assert info["match"] in got, (name, level, got[-3:])
        if "matches" in info:
            assert got == info["matches"], (name, level, got)
        if "matches_at" in info:
            assert info["matches_at"] in got, (name, level)
        if "matches_in" in info:
            assert set(info["matches_in"]) <= set(got) and len(got) == info["count"], (name, level, got)
        for p, d, found in info.get("grid", ()):
            assert ((p + d, d, 20) in got) == found, (name, level, p, d)
            if not found:   # (a key in slot 0 is found from its second byte on, where the distance allows)
                behind = [(p + d + 1, d, 19)] if d <= 32767 else []
                assert [m for m in got if p + d - 4 <= m[0] < p + d + 20] == behind, (name, level, p, d)
                if d == 32768 and p % 32768:
                    assert stats[p + d][2] == "offset0", (name, level, stats[p + d])
        if "period" in info:
            p = info["period"]
            assert got[0][0] == p + 1 and all(m[1] == p for m in got), (name, level)
            assert all(m[2] == 258 for m in got[:-1]) and all(b[0] == a[0] + 258 for a, b in zip(got, got[1:])), (name, level)
            assert got[-1][0] + got[-1][2] >= len(src) - 4


def test_block_borders():
    """a repeat that crosses a block's end is clipped there; a string of one block's last bytes is not found from the
    next block (fresh `head`); the same string inside one block is"""
    for name, src, levels, _ in CASES:
        if not name.startswith("C/block/"):
            continue
        sizes = pc.CHAIN_BLOCK_SIZES if name == "C/block/borders_32768_65536" else (pc.FULL_BLOCK,)
        for size in sizes:
            for level in levels:
                per_block = {}
                for start, length in blocks_of(src, size):
                    per_block[start] = cm.model(src, level, start, length)
                    assert per_block[start] == oracle_matches(src, level, start, length), (name, level, size, start)
                for at in pc.chain_case_info[name]["borders"]:
                    if at % size == 0:
                        assert (size - 10, 1990, 10) in per_block[at - size], (name, level, size, at)
                        assert not [m for m in per_block[at] if m[0] < 100], (name, level, size, at)
                    else:
                        start = at - at % size
                        assert (at - 10 - start, 1990, 40) in per_block[start] and (at + 50 - start, 90, 30) in per_block[start]


def test_device_structure_cells():
    full = {c[0]: c for c in CASES}
    # crowded: at least 5000 matches in the second fragment (ZH_MAX_MATCHES_PER_FRAG is 8192, the ceiling here 32768 / 6)
    name, src, levels, _ = full["C/crowded/fragment_of_5459_matches"]
    for level in levels:
        got, _ = run(name, src, level)
        assert sum(1 for m in got if pc.FRAG <= m[0] < 2 * pc.FRAG) >= 5000, level
    # classes and tiles: tile 0 in one class, a class that begins in tile 2, an empty class
    name, src, levels, _ = full["C/classes/three_tiles"]
    cls = pc.chain_classes(src)
    assert len(cls) == 3 * pc.CHAIN_TILE + 100
    assert len(set(cls[:pc.CHAIN_TILE].tolist())) == 1
    firsts = {c: int(np.flatnonzero(cls == c)[0]) for c in set(cls.tolist())}
    assert any(at >= 2 * pc.CHAIN_TILE for at in firsts.values())
    assert len(firsts) < 32
    # tags: candidates of the searcher's hash and tag that match fewer than five bytes
    name, src, levels, _ = full["C/tags/equal_tag_other_bytes"]
    info = pc.chain_case_info[name]
    s5 = info["searcher5"]
    same = [c for c in info["candidates"] if pc.chain_tag(c) == pc.chain_tag(s5) and pc.chain_hash(c) == pc.chain_hash(s5) and c != s5]
    assert len(same) >= 1 and all(c in src for c in same)
    assert all(cm.match_length(c + s5, 0, 5, 10) < 5 for c in same)
    # spill: the matches end 0, 1, 2 and 257 bytes behind the border, or start 1 and 5 bytes in front of it
    ends = sorted(i["matches_at"][0] + i["matches_at"][2] - pc.FRAG for n, i in pc.chain_case_info.items() if "/spill/" in n)
    assert ends == [0, 1, 2, 95, 257]


def test_hash_words():
    for h in (0, 1, 77777, 131071):
        assert {pc.chain_hash(pc.chain_word(h, low)) for low in (0, 1, 12345, 32767)} == {h}
    assert len({pc.chain_word(5, low) for low in range(32768)}) == 32768


def test_chain_small_subset_and_sizes():
    full = {c[0]: c for c in CASES}
    assert max(len(c[1]) for c in CASES) == pc.FULL_BLOCK + 70000
    assert sum(len(c[1]) for c in CASES) < 8 << 20
    assert sum(len(c[1]) * len(c[2]) for c in CASES) < 24 << 20   # what a device run compresses
    small = pc.chain_crafted_inputs(small=True)
    cell = lambda name: name.split("/")[1]
    assert {cell(c[0]) for c in small} == {cell(c[0]) for c in CASES}
    for name, src, levels, kills in small:
        assert full[name][1] == src and set(levels) <= set(full[name][2]) and kills <= full[name][3], name
        assert set(levels) <= set(pc.CHAIN_DEVICE_LEVELS) and len(src) <= 110000, name
    for c in {cell(c[0]) for c in small}:   # every cell with wide records and with narrow ones
        mine = {lv for n, _, levels, _ in small if cell(n) == c for lv in levels}
        assert mine == {2, -1, 9}, (c, mine)
    assert sum(len(c[1]) * len(c[2]) for c in small) < 3 << 20
