"""The parallel BestSpeed parse's rule (contract mode: zh_set_l1_parse(ctx, 1), zippy_amd/csrc/zh_l1p_match.hip) as
one serial function in plain Python, with named single-decision mutants.  No device code and nothing of the kernel's
structure (no chunks, no waves, no guessed entries): the kernel claims that its fixed point is this walk, and
check_l1p_tokens (parity_cases.py) holds its tokens against it; tests/test_l1p_craft.py shows that each crafted input
of family P tells the mutants it names from the rule.

The rule, for one fragment of n bytes (a buffer is cut into 4 MiB blocks and those into 32 KiB fragments):
  * hash and table: w(p) is the little-endian 32-bit word at min(p, n - 4), for p in 0 .. 64 * ceil(n / 64) - 1;
    h = w * 0x1e35a7bd mod 2^32, slot = h >> 18, tag = (h >> 2) & 0xffff, h30 = h >> 2.  The table is empty at the
    start of every fragment; positions enter in ascending order, every one of them; raw(p) is the entry of slot(p)
    just before p enters it (0: none), and the entry becomes max(entry, p << 16 | tag(p)).  Nothing happens at all
    when n < 16.
  * candidate of p: c = raw >> 16, valid if c < p and the tags agree; if p >= 2 and h30(p) == h30(p - 1), c = p - 1;
    c == 0 means none (position 0 is never a candidate).
  * length: 0 unless p + 16 <= n and there is a candidate; else the common prefix of p and c, capped at
    min(n - p, 258); a length below 4 counts as 0.
  * parse: greedy from p = 0; a length m > 0 gives the token (p, p - c, m) and p += m, else a literal and p += 1.

Mutants that no input can tell from the rule (test_l1p_craft.py runs them over every case all the same):
  * `min3` (a length of 3 counts) and `no_tag` (the tags are not compared): a candidate is read from the position's
    own slot, so the 14 slot bits of its h agree; with the tag the 30 bits of h30 do.  Two DIFFERENT words with equal
    h30 have products that differ by d in 1..3, so the words differ by d * MUL^-1 mod 2^32; MUL^-1 is odd, so
    d * MUL^-1 is no multiple of 4, let alone of 256: their FIRST bytes differ and the common prefix is 0.  Hence a
    valid candidate either has the position's four bytes (length >= 4) or matches 0 bytes: never 3 (`min3`).  And a
    candidate whose tag does not agree has another word, a common prefix of at most 3, which counts as 0 with the
    tag test or without (`no_tag`).  The run rule's p - 1 has an equal h30 itself, so the same holds for it.
  * `run_from1` (the run rule from p >= 1): at p = 1 it gives c = 0, which already means none.
  * `no_run` (no run rule) and `run_from3` (from p >= 3), under ascending insertion: when h30(p) == h30(p - 1), p - 1
    entered slot(p) right before p with p's tag, and nothing entered in between, so raw(p) >> 16 already is p - 1.
    The run rule only matters to a device that serves the lanes of a 64-position step in another order."""
import numpy as np

FRAG = 32768
BLOCK = 4194304
MIN_MATCH = 4
MAX_MATCH = 258
TAIL = 16
HASH_MUL = 0x1e35a7bd
STEP = 64

MUTANTS = ("tail15", "tail17", "lim257", "lim259", "lim_past_frag", "min5", "pos0", "visited_only", "step_granular",
           "table_survives")
INEXPRESSIBLE = ("min3", "no_tag", "run_from1", "no_run", "run_from3")


def fragments(n):
    """-> [(start, length)] of a buffer of n bytes: 4 MiB blocks, each cut into 32 KiB fragments"""
    return [(o, min(FRAG, min(b + BLOCK, n) - o)) for b in range(0, n, BLOCK) for o in range(b, min(b + BLOCK, n), FRAG)]


def hashes(frag):
    """h of every position that enters the table: 0 .. 64 * ceil(n / 64) - 1, the word at min(p, n - 4)"""
    n = len(frag)
    a = np.frombuffer(frag, np.uint8).astype(np.uint32)
    w = a[:n - 3] | a[1:n - 2] << 8 | a[2:n - 1] << 16 | a[3:] << 24
    at = np.minimum(np.arange((n + STEP - 1) // STEP * STEP), n - 4)
    return (w[at] * np.uint32(HASH_MUL)).tolist()


def common_prefix(buf, a, b, cap):
    """bytes of buf[b:b + cap] that equal buf[a:] (a < b; the two may overlap)"""
    if buf[a:a + cap] == buf[b:b + cap]:
        return cap
    k = 0
    while buf[a + k:a + k + 16] == buf[b + k:b + k + 16]:
        k += 16
    while buf[a + k] == buf[b + k]:
        k += 1
    return k


def fragment(src, start, n, tab, mutant=None, every=False):
    """One fragment, src[start:start + n], through the table `tab` (a list of 16384 entries, None: empty).
    -> [(position in the fragment, offset, length)]; every: the length at EVERY position instead (0 or 4..258), a list
    of n entries -- what the parse would find wherever it came by."""
    out, lens = [], [0] * n
    if n < TAIL:
        return lens if every else out
    frag = src[start:start + n]
    hs = hashes(frag)
    tail = {"tail15": TAIL - 1, "tail17": TAIL + 1}.get(mutant, TAIL)
    cap = {"lim257": MAX_MATCH - 1, "lim259": MAX_MATCH + 1}.get(mutant, MAX_MATCH)
    min_len = {"min5": 5, "min3": 3}.get(mutant, MIN_MATCH)
    run_from = {"run_from1": 1, "run_from3": 3, "no_run": 1 << 30}.get(mutant, 2)
    pending = []   # step_granular: what entered in this step
    at = 0         # the parse stands here
    for p in range(len(hs)):
        h = hs[p]
        slot, tag, own = h >> 18, (h >> 2) & 0xffff, p << 16 | (h >> 2) & 0xffff
        if mutant == "step_granular" and p % STEP == 0:
            for s, v in pending:
                if tab[s] is None or v > tab[s]:
                    tab[s] = v
            pending = []
        raw = tab[slot]
        if mutant == "visited_only" and p != at:
            pass
        elif mutant == "step_granular":
            pending.append((slot, own))
        elif raw is None or own > raw:
            tab[slot] = own
        if p >= n or (p != at and not every):
            continue
        c = None
        if raw is not None and raw >> 16 < p and (raw & 0xffff == tag or mutant == "no_tag"):
            c = raw >> 16
        if p >= run_from and h >> 2 == hs[p - 1] >> 2:
            c = p - 1
        if c == 0 and mutant != "pos0":
            c = None
        m = 0
        if p + tail <= n and c is not None:
            if mutant == "lim_past_frag":
                m = common_prefix(src, start + c, start + p, min(len(src) - start - p, cap))
            else:
                m = common_prefix(frag, c, p, min(n - p, cap))
            if m < min_len:
                m = 0
        lens[p] = m
        if p == at:
            if m:
                out.append((p, p - c, m))
                at += m
            else:
                at += 1
    return lens if every else out


def model(src, mutant=None):
    """-> [(position, offset, length)] of the whole buffer, fragment by fragment"""
    assert mutant is None or mutant in MUTANTS or mutant in INEXPRESSIBLE, mutant
    src = bytes(src)
    out = []
    tab = [None] * 16384
    for start, n in fragments(len(src)):
        if mutant != "table_survives":
            tab = [None] * 16384
        out += [(start + p, off, m) for p, off, m in fragment(src, start, n, tab, mutant)]
    return out


def literals(src, matches):
    """the literals that the matches of a buffer leave, once they are shown to be a parse at all: ascending, not
    overlapping, inside their fragments, each a true copy"""
    at = lits = 0
    for p, off, m in matches:
        assert p >= at and MIN_MATCH <= m <= MAX_MATCH and 1 <= off <= p % FRAG and p % FRAG + m <= FRAG, (p, off, m)
        assert p + m <= len(src) and src[p:p + m] == bytes(src[p + i - off] for i in range(m)), (p, off, m)
        lits += p - at
        at = p + m
    return lits + len(src) - at
