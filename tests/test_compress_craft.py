"""The crafted compress inputs of parity_cases.crafted_inputs() on the CPU, before any device sees them: the oracle
alone says that every input reaches the corner of the encoder it is built for -- the literal counts around the stored
threshold, the block types, the cells of the code lengths' run-length coding, the stretches of 14- and 15-bit codes,
the BestSpeed matcher's edges.  A generator that silently stops reaching a cell fails here."""
import zlib

import numpy as np

import oracle
import parity_cases as pc

STORED, FIXED, DYNAMIC = 0, 1, 2


def _cases(family, small=False):
    return [c for c in pc.crafted_inputs(small) if c[0].startswith(family + "/")]


def test_threshold_lengths_disagree():
    """the premise of family S: where the float32 product and exact arithmetic part"""
    n = np.arange(1, pc.FULL_BLOCK + 1, dtype=np.int64)
    t = (n.astype(np.float32) * np.float32(0.98)).astype(np.int64)
    differ = n[t != n * 98 // 100]
    assert differ[0] == pc.S_LEN_FIRST and pc.S_LEN_SECOND in differ and pc.FULL_BLOCK in differ
    assert pc.S_LEN_FIRST < pc.S_LEN_SECOND < 1 << 20
    for length in (pc.S_LEN_FIRST, pc.S_LEN_SECOND, pc.FULL_BLOCK):
        assert pc.stored_threshold(length) == t[length - 1] == length * 98 // 100 + 1


def test_stored_family_sits_on_the_threshold():
    """every (level, length) pair has inputs with T - 1, T and T + 1 literals in the first block and one on the exact
    threshold len * 98 // 100; the oracle stores the block exactly from T on; behind a stored and behind a compressed
    full block there is a fixed (level 1), a dynamic (level 9) and a stored short block"""
    seen, second = {}, set()
    for name, src, levels, formats in _cases("S"):
        assert src is not None, (name, "not found")
        level = levels[0]
        target = int(name.split("nlit")[1].split("_")[0])
        total = min(len(src), pc.FULL_BLOCK)
        types, nlit = pc.block_types(src, level)
        assert nlit == target, name
        t = pc.stored_threshold(total)
        assert (types[0] == STORED) == (nlit >= t), name
        seen.setdefault((level, total), set()).add(target - t)
        if len(src) > pc.FULL_BLOCK:
            assert len(src) == pc.FULL_BLOCK + 1000
            assert (types[0] == STORED) == (len(types) == 66) and types[0] in (STORED, DYNAMIC), name  # 65 pieces of 65 535 bytes
            second.add((level, types[0] == STORED, types[-1]))
            assert types[-1] == (STORED if name.endswith("noise") else FIXED if level == 1 else DYNAMIC), name
    want = {(1, pc.S_LEN_FIRST), (-1, pc.S_LEN_FIRST), (1, pc.S_LEN_SECOND), (1, pc.FULL_BLOCK), (9, pc.FULL_BLOCK)}
    assert set(seen) == want
    for key, offsets in seen.items():
        assert offsets == {-1, 0, 1}, key  # (-1 is the exact threshold at all three lengths)
        assert key[1] * 98 // 100 - pc.stored_threshold(key[1]) == -1
    assert second == {(1, True, FIXED), (1, True, STORED), (1, False, FIXED), (1, False, STORED),
                      (9, True, DYNAMIC), (9, True, STORED), (9, False, DYNAMIC), (9, False, STORED)}


def test_fixed_dynamic_family():
    """13 lengths x 3 kinds at every level, all three containers at levels 1, 6, 7 and 9; the oracle's block types:
    fixed up to 2 048 bytes and level 6, dynamic beyond either, tiny dynamic blocks at levels 7 to 9"""
    runs = {}
    for name, src, levels, formats in _cases("F"):
        key = name.replace("/gzip", "")
        for level in levels:
            assert level not in runs.setdefault(key, {})
            runs[key][level] = formats
    assert len(runs) == 39 and {len(dict(pc.f_inputs())[k]) for k in runs} == set(pc.F_LENGTHS)
    for key, by_level in runs.items():
        assert set(by_level) == set(pc.ALL_LEVELS), key
        for level, formats in by_level.items():
            assert set(formats) == (set(pc.FORMATS) if level in (1, 6, 7, 9) else {oracle.dfGzip}), (key, level)
    tiny_dynamic = set()
    for name, src in pc.f_inputs():
        for level in pc.ALL_LEVELS:
            (btype,), nlit = pc.block_types(src, level)
            if level == 0 or (level != -2 and nlit >= pc.stored_threshold(len(src))):
                assert btype == STORED, (name, level)
            else:
                assert btype == (FIXED if level <= 6 and len(src) <= 2048 else DYNAMIC), (name, level)
                if btype == DYNAMIC and len(src) <= 16:
                    tiny_dynamic.add((len(src), level))
            if len(src) >= 2047 and level != 0:
                assert btype != STORED, (name, level)  # all three kinds cross the fixed / dynamic border compressed
    assert tiny_dynamic == {(n, level) for n in (14, 15, 16) for level in (7, 8, 9)}
    for n in (0, 1, 2, 3):   # lz77.nim:54-56: nothing to match in a block of at most three bytes
        assert pc.block_types(b"\xe7" * n, 9) == ([STORED], n)


def test_run_length_family_reaches_every_cell():
    """The cells of the code lengths' run-length coding, recomputed from oracle.block_tokens and oracle.huffman_codes.
    n_litlen is never below 258 (the reference counts max(highest, 257) + 1 codes) and n_dist never below 3, so at
    level -2 a zero always stands between the end-of-block symbol's length and the distance lengths 1, 1, 0: the run
    that crosses from one array into the other comes from inputs with matches (length symbol 285 and distance codes
    0 and 1, all of length 1).  The smallest HCLEN + 4 these inputs reach is 14.
    The array ends in the distance lengths, whose last entry is either the highest used code's (non-zero) or the zero
    that fills n_dist up to 3: a last run of zeros is one long, never the three the closed form starts at; the last
    run of non-zero lengths that reaches the closed form (four or more) is R/eight_periods'."""
    zero_runs, nonzero_runs, heads, hclen4, shapes = set(), {}, set(), set(), set()
    crossing, swallowed, close_at_end, near_dist3, far, third_word = [], [], [], [], [], []
    for name, src, levels, formats in _cases("R"):
        for level in levels:
            cells = pc.header_cells(src, level)
            n_litlen, total = cells["n_litlen"], cells["n_litlen"] + cells["n_dist"]
            assert sum(r[2] for r in cells["runs"]) == total == len(cells["lens"])
            for start, value, length in cells["runs"]:
                heads.add(start)
                if value == 0:
                    zero_runs.add(length)
                else:
                    nonzero_runs.setdefault(length, set()).add(value)
                if start < n_litlen < start + length:
                    crossing.append((name, level, value, length))
                for g in range(1, 5):
                    if start < 64 * g and start + length >= 64 * g + 64:
                        swallowed.append((name, value != 0, g))
            start, value, length = cells["runs"][-1]
            close_at_end.append((value != 0, length))
            if cells["cl_lens"].get(2):   # the sixteenth 3-bit length, at header bits 62 .. 64, is not zero
                assert cells["hclen4"] >= 16 and pc.CLCL_ORDER[15] == 2
                third_word.append(name)
            hclen4.add(cells["hclen4"])
            shapes.add((n_litlen, cells["n_dist"]))
            matches, _ = pc.token_matches(oracle.block_tokens(src, level)[0])
            if level == -2:
                assert not matches and n_litlen == 258 and cells["n_dist"] == 3 and cells["lens"][-3:] == [1, 1, 0], name
            if matches and cells["n_dist"] == 3 and max(m[1] for m in matches) <= 4:
                near_dist3.append((name, level))
            if (n_litlen, cells["n_dist"]) == (286, 30) and any(m[2] == 258 and m[1] >= 24577 for m in matches):
                far.append(level)
    assert zero_runs >= set(pc.R_ZERO_RUNS), sorted(set(pc.R_ZERO_RUNS) - zero_runs)
    assert set(nonzero_runs) >= set(pc.R_NONZERO_RUNS), sorted(set(pc.R_NONZERO_RUNS) - set(nonzero_runs))
    big = sorted(n for n in nonzero_runs if n >= 130)
    assert {(n - 1) % 6 >= 3 for n in big} == {True, False}, big   # a large quotient with either kind of remainder
    values = set().union(*nonzero_runs.values())
    assert values == set(range(1, 16))
    assert heads >= set(pc.R_HEADS)
    assert any(nz for _, nz, _ in swallowed) and any(not nz for _, nz, _ in swallowed)
    assert {g for _, _, g in swallowed} == {1, 2, 3}
    assert any(value != 0 for _, _, value, _ in crossing), "no run crosses from the literal/length lengths into the distances'"
    assert max(n for nz, n in close_at_end if nz) >= 4, "no last run of four or more equal non-zero lengths"
    assert {n for nz, n in close_at_end if not nz} == {1}
    assert min(shapes) == (258, 3) and (286, 30) in shapes and sorted(far) == [1, 9]
    assert near_dist3
    assert min(hclen4) == 14 and {18, 19} <= hclen4, sorted(hclen4)
    assert third_word, "no header whose sixteenth 3-bit length, the one across two header words, is non-zero"


def test_dyadic_builder_dictates_the_lengths():
    for name, (layout, top) in pc.r_layouts().items():
        src, lens = pc.dyadic_input(layout, top, 77)
        assert 2048 < len(src) == (1 << top) - 1, name
        got = pc.header_cells(src, -2)["lens"]
        assert got[256] == top and got[:256] == [lens.get(v, 0) for v in range(256)], name


def test_long_literal_codes():
    """E: two stretches of at least 1 536 consecutive positions whose bytes all have 14- or 15-bit codes, the first at
    an offset that is no multiple of 512, the second across a fragment border; the length limit ran"""
    name, src, levels, formats = _cases("E")[0]
    assert name == "E/long_literal_codes"
    assert levels == (-2,) and 200000 < len(src) <= pc.FULL_BLOCK
    _, freq, _, _ = oracle.block_tokens(src, -2)
    lens = oracle.huffman_codes(freq, 257, 15)[1]
    assert max(lens) == 15
    assert pc.huffman_depth(freq) > 15, "the unlimited tree is not deeper than 15"
    wide = np.isin(np.frombuffer(src, np.uint8), [v for v in range(256) if lens[v] >= 14]).astype(np.int8)
    edges = np.flatnonzero(np.diff(np.concatenate(([0], wide, [0]))))
    stretches = [(a, b - a) for a, b in zip(edges[::2], edges[1::2]) if b - a >= 1536]
    assert [s[0] for s in stretches] == [pc.E_FIRST_AT, pc.E_SECOND_AT] and all(s[1] >= 1536 for s in stretches)
    assert stretches[0][0] % 512 != 0
    a, n = stretches[1]
    assert a // pc.FRAG != (a + n - 1) // pc.FRAG
    bits = sum(int(lens[b]) for b in src[pc.E_FIRST_AT:pc.E_FIRST_AT + 512])
    assert bits >= 14 * 512   # (512 positions of 15 bits are 7 680 bits, the emission's flush threshold)


def test_long_match_tokens():
    """E: at level 1 and at level 9 twelve match tokens of at least 41 bits (length code + 5 extra bits + distance code
    + 13 extra bits) back to back over 2 400 positions, from the oracle's tokens and code lengths; the issue asks for
    40 bits over 512 positions"""
    cases = {c[0]: c for c in _cases("E")}
    for level in (1, 9):
        name, src, levels, formats = cases["E/long_match_tokens_level%d" % level]
        assert levels == (level,) and len(src) <= pc.FULL_BLOCK
        span, tokens, bits = pc.widest_match_stretch(src, level)
        print(name, span, tokens, bits)
        assert span >= 512 and bits >= 40, (name, span, tokens, bits)
        assert (span, tokens, bits) == (2400, 12, 41), name
        assert pc.block_types(src, level)[0] == [DYNAMIC]


def test_matcher_family():
    """M: the fragment lengths, the tails, and what the oracle's BestSpeed tokens say about the rest"""
    cases = {c[0]: c[1] for c in _cases("M")}
    last = {}
    for name, src in cases.items():
        if name.startswith("M/frag_"):
            n = int(name.split("_")[1])
            behind = int(name.rsplit("_", 1)[1])
            assert len(src) == behind * pc.FRAG + n
            last.setdefault(n, set()).add((name.split("_")[2], behind))
    assert set(last) == set(pc.M_TABLE_BORDERS) and all({k for k, _ in v} == {"text", "runs"} for v in last.values())
    assert {b for v in last.values() for _, b in v} == {0, 1, 2}
    assert {len(src) for name, src in cases.items() if name.startswith("M/tail_")} == \
        {f * pc.FRAG + k for f in (1, 2) for k in range(1, 17)}
    tokens = {}
    for name, src in cases.items():
        matches, covered = pc.token_matches(oracle.block_tokens(src, 1)[0])
        assert covered == len(src)
        for pos, offset, length in matches:
            assert offset <= pos % pc.FRAG, (name, "a match reaches into the fragment before")
            assert pos // pc.FRAG == (pos + length - 1) // pc.FRAG, (name, "a match crosses the fragment border")
            assert pos % pc.FRAG + 15 <= min(pc.FRAG, len(src) - pos // pc.FRAG * pc.FRAG), (name, "a match starts in the last 15 bytes")
        tokens[name] = matches
    first = [m for m in tokens["M/position_0_first_fragment"] if m[0] == m[1] and m[0] > 4]
    later = [m for m in tokens["M/position_0_later_fragment"] if m[0] >= pc.FRAG and m[0] - pc.FRAG == m[1] and m[1] > 4]
    assert first and later, "position 0 of the fragment is nobody's candidate"
    assert [m[2] for m in tokens["M/run_one_byte_fragment"]] == [258] * 127 and tokens["M/run_one_byte_fragment"][0][:2] == (1, 1)
    assert [m[1:] for m in tokens["M/run_period_2_fragment"]][1:] == [(258, 258)] * 126
    assert tokens["M/run_period_2_fragment"][-1][0] + 258 == pc.FRAG   # the last match ends at the fragment's end
    ends = {gap: max(m[0] + m[2] for m in tokens["M/run_ends_%d_before_end" % gap] if m[0] < pc.FRAG) for gap in (0, 14, 15, 16)}
    assert ends == {gap: pc.FRAG - gap for gap in ends}, ends   # the last match stops where the run does
    border = tokens["M/run_crosses_border"]
    assert any(m[0] + m[2] == pc.FRAG for m in border) and any(m[0] == pc.FRAG + 1 and m[1] == 1 for m in border)
    stride = tokens["M/probe_stride"]
    assert not [m for m in stride if m[0] < 32768] and len([m for m in stride if 40000 <= m[0] < 70000]) > 1000
    twice = tokens["M/fragment_twice"]
    assert [(p - pc.FRAG, o, n) for p, o, n in twice if p >= pc.FRAG] == [m for m in twice if m[0] < pc.FRAG]


def test_small_subset_and_sizes():
    full = {c[0]: c for c in pc.crafted_inputs(False)}
    assert max(len(c[1]) for c in full.values()) == pc.FULL_BLOCK + 1000
    assert sum(len(c[1]) for c in full.values()) < 64 << 20
    small = pc.crafted_inputs(True)
    for name, src, levels, formats in small:
        assert full[name][1] == src and set(formats) <= set(full[name][3]), name
        assert len(src) <= 400000, name
    assert {c[0].split("/")[0] for c in small} == {"S", "F", "R", "E", "M"}
    assert {c[0] for c in small if c[0][0] in "RE"} == {name for name in full if name[0] in "RE"}  # every header cell
    assert sum(len(c[1]) for c in small) < 3 << 20
    blob = oracle.compress(full["R/zero_255"][1], -2, oracle.dfZlib)
    assert zlib.decompress(blob) == full["R/zero_255"][1]
