"""The reference's hash-chain matcher (lz77.nim:10-130 encodeLz77, as oracle/zippy_oracle.c restates it) in plain
Python, statement for statement, with named single-decision mutants.  No device code: tests/test_chain_craft.py holds
the model against the oracle's tokens and shows that each crafted input of family C tells the mutants it names from
the reference.

Mutants left out because no input can tell them from the reference:
  * `offset <= prev_offset` ends the walk (instead of `<`), while the self-loop test stands: two consecutive
    candidates of equal offset are the same window slot, hash_pos == chain[hash_pos], and the self-loop test has
    already ended the walk on the first of them.  Likewise "no self-loop test" while `offset < prev_offset` stands:
    a slot that links to itself is visited again with an equal offset, an equal match length (no improvement, no
    cut), and so on until `tries` runs out -- nothing it finds is new.
  * "links older than the window are dropped": `head[h]` always names the newest position of hash h, and each link
    the next older one, so the positions of hash h inside the window are exactly the candidates in front of the
    first link that is older than the window.  Behind it the walk reads slots that later positions own.  Such an
    owner either has another hash -- another first word, a match of at most three bytes, which is not accepted
    (> 4), cuts nothing (good >= 4) and reaches no `nice` (>= 8), and whose own links lead to more of the kind -- or
    is one of the candidates already seen, which ends the walk (a smaller offset, or the self-loop test).
  * `insert_last4` (positions with pos + 4 >= block_end are inserted and searched): the limit of such a search is
    block_end, at most four bytes away, and a match is accepted only from five bytes on; what such a position inserts
    is read only by the (at most three) positions behind it, whose searches are as short.  `head` and `chain` are
    dropped at the block's end.  No token changes."""
import numpy as np

WINDOW = 32768
MIN_MATCH = 4
MAX_MATCH = 258
HASH_MUL = 0x1e35a7bd
HASH_BITS = 17

# internal.nim:177-189: (good, nice, chain) of zlib's configuration_table (`lazy` is unused: the parse is greedy)
CONFIG = {1: (4, 8, 4), 2: (4, 16, 8), 3: (4, 32, 32), 4: (4, 16, 16), 5: (8, 32, 32), 6: (8, 128, 128),
          7: (8, 256, 256), 8: (32, 258, 1024), 9: (32, 258, 4096)}

MUTANTS = ("chain+1", "chain-1", "good_gt", "shr1", "cut_always", "nice_gt", "ge_longest", "min4", "min6",
           "no_sentinel", "wrap_eq", "no_skip_insert", "limit_259", "limit_ignores_block_end", "head_survives_block",
           "tag4", "config-1", "config+1")


def config(level, mutant=None):
    level = 6 if level == -1 else level
    if mutant == "config-1":
        level -= 1
    elif mutant == "config+1":
        level += 1
    return CONFIG[level]


def has_mutant(level, mutant):
    """config-1 / config+1 exist where the neighbouring level has a tuple of its own"""
    level = 6 if level == -1 else level
    if mutant == "config-1":
        return level - 1 in CONFIG and CONFIG[level - 1] != CONFIG[level]
    if mutant == "config+1":
        return level + 1 in CONFIG and CONFIG[level + 1] != CONFIG[level]
    return True


def hashes(src, start, end):
    """HASH4 of every position in [start, end) whose four bytes lie inside src"""
    n = max(0, min(end, len(src) - 3) - start)
    if n == 0:
        return []
    a = np.frombuffer(src, np.uint8, n + 3, start).astype(np.uint32)
    w = a[:n] | a[1:n + 1] << 8 | a[2:n + 2] << 16 | a[3:n + 3] << 24
    return ((w * np.uint32(HASH_MUL)) >> np.uint32(32 - HASH_BITS)).tolist()


def match_length(src, s1, s2, limit):
    """determineMatchLength: bytes of src[s2:limit] that equal src[s1:]"""
    n = limit - s2
    k = 0
    while k < n and k < 8:
        if src[s1 + k] != src[s2 + k]:
            return k
        k += 1
    if src[s1:s1 + n] == src[s2:limit]:
        return n
    lo, hi = k, n  # src[s1:s1+lo] matches, src[s1:s1+hi] does not
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if src[s1 + lo:s1 + mid] == src[s2 + lo:s2 + mid]:
            lo = mid
        else:
            hi = mid
    return lo


def model(src, level, block_start=0, block_len=None, mutant=None, stats=None, block_size=None):
    """-> [(position in the block, offset, length)] of the block src[block_start:block_start + block_len].
    block_size: under `head_survives_block`, the length of the blocks in front of this one (default: block_len)."""
    assert mutant is None or mutant in MUTANTS
    src = bytes(src)
    if block_len is None:
        block_len = len(src) - block_start
    good, nice, chain_len = config(level, mutant)
    if mutant == "chain+1":
        chain_len += 1
    elif mutant == "chain-1":
        chain_len -= 1
    min_len = {"min4": 3, "min6": 5}.get(mutant, MIN_MATCH)
    max_len = 259 if mutant == "limit_259" else MAX_MATCH
    head = [0] * (1 << HASH_BITS)
    chain = [0] * WINDOW
    if mutant == "head_survives_block":  # the blocks in front leave their tables behind
        size = block_size or block_len
        for start in range(block_start % size, block_start, size):
            _block(src, start, size, good, nice, chain_len, min_len, max_len, head, chain, mutant, None)
    return _block(src, block_start, block_len, good, nice, chain_len, min_len, max_len, head, chain, mutant, stats)


def _block(src, block_start, block_len, good, nice, chain_len, min_len, max_len, head, chain, mutant, stats):
    out = []
    if MIN_MATCH >= block_len:
        return out
    block_end = block_start + block_len
    hs = hashes(src, block_start, block_end)
    pos = block_start
    while pos < block_end:
        if pos + MIN_MATCH >= block_end:
            break
        window_pos = (pos - block_start) & (WINDOW - 1)
        h = hs[pos - block_start]
        chain[window_pos] = head[h]
        head[h] = window_pos

        hash_pos = chain[window_pos]
        limit = min(block_end, pos + max_len)
        if mutant == "limit_ignores_block_end":
            limit = min(len(src), pos + max_len)
        tries = chain_len
        prev_offset = longest_offset = longest_len = 0
        tried = cuts = 0
        why = "tries"
        while tries > 0:
            if hash_pos == 0 and mutant != "no_sentinel":
                why = "empty"
                break
            tries -= 1
            if hash_pos < window_pos or (hash_pos == window_pos and mutant != "wrap_eq"):
                offset = window_pos - hash_pos
            else:
                offset = window_pos - hash_pos + WINDOW
            if offset <= 0:
                why = "offset0"
                break
            if offset < prev_offset:
                why = "descending"
                break
            prev_offset = offset
            tried += 1
            assert pos - offset >= 0
            match_len = match_length(src, pos - offset, pos, limit)
            if mutant == "tag4" and match_len < 5:
                match_len = 0
            if match_len > longest_len or (mutant == "ge_longest" and match_len == longest_len):
                if match_len > good if mutant == "good_gt" else match_len >= good:
                    tries >>= 1 if mutant == "shr1" else 2
                    cuts += 1
                longest_len = match_len
                longest_offset = offset
            elif mutant == "cut_always" and match_len >= good:
                tries >>= 2
                cuts += 1
            if longest_len > nice if mutant == "nice_gt" else longest_len >= nice:
                why = "nice"
                break
            if hash_pos == chain[hash_pos]:
                why = "self"
                break
            hash_pos = chain[hash_pos]
        if stats is not None:
            stats.append((pos - block_start, tried, why, longest_len, cuts))

        if longest_len > min_len:
            out.append((pos - block_start, longest_offset, longest_len))
            for _ in range(1, longest_len):
                pos += 1
                if pos + MIN_MATCH < block_end and mutant != "no_skip_insert":
                    window_pos = pos & (WINDOW - 1)  # the absolute position, as lz77.nim:123 has it
                    h = hs[pos - block_start]
                    chain[window_pos] = head[h]
                    head[h] = window_pos
        pos += 1
    return out
