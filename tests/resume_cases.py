"""Cases of zh_uncompress_resume_batch shared by tests/test_emu_resume.py (fiber emulator) and tests/test_gpu_resume.py
(MI355X).  Streams come from tests/deflate_craft.py, from Python's zlib over synth.py's data and from
tests/parity_cases.py; every expectation -- output, consumed, why, status and the state byte for byte -- is the model's
(tests/resume_model.py), and every case asserts its premise with the model before the engine runs."""
import functools
import random
import struct
import zlib

import deflate_craft as dc
import resume_model as rm
import seek_cases as sc
import synth

OK, CHECKSUM, SIZE, INVALID_BUFFER, END_OF_BUFFER, ARGUMENT = 0, 8, 9, 13, 15, 22
BIG = 1 << 20
FORMATS = (rm.DF_DEFLATE, rm.DF_ZLIB, rm.DF_GZIP)


def wrap(raw, plain, fmt, name=b"a.txt"):
    if fmt == rm.DF_ZLIB:
        return b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(plain))
    if fmt == rm.DF_GZIP:
        return (b"\x1f\x8b\x08\x08\0\0\0\0\0\x03" + name + b"\0" + raw
                + struct.pack("<II", zlib.crc32(plain), len(plain) & 0xffffffff))
    return raw


@functools.lru_cache(maxsize=None)
def small_raw():
    """Stored blocks (one of them empty), fixed blocks of 19 bits each -- so that block boundaries fall on every bit of
    a byte --, a dynamic block whose distance code has no codes at all (every pattern, the all-zero one too, is
    unclaimed), one with a single distance code of one bit, and zlib's own dynamic blocks behind a sync and a full
    flush -> (raw deflate, plaintext)"""
    text = synth.gen_mix_buffer(5, 8000).tobytes()
    s = dc.Stream()
    s.stored(text[:300], False)
    s.stored(b"", False)
    for j in range(9):
        s.fixed_block(False)
        s.lit(200 + j)
        s.eob()
    s.fixed_block(False)
    for b in text[300:340]:
        s.lit(b)
    s.match(30, 200)
    s.match(258, 1)
    s.match(3, 339)
    s.eob()
    lit_lens = [0] * 257
    for sym in (97, 98, 99, 100):
        lit_lens[sym] = 3
    lit_lens[256] = 1
    s.dynamic_block(lit_lens, [0], False)
    for b in b"abcdabcddcba":
        s.lit(b)
    s.eob()
    lit_lens = [0] * 286
    for sym in (102, 103, 260, 285):
        lit_lens[sym] = 3
    lit_lens[101] = lit_lens[256] = 2
    s.dynamic_block(lit_lens, [1], False)
    for b in b"efgfe":
        s.lit(b)
    s.match(6, 1)
    s.match(258, 1)
    s.eob()
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    s.stored(b"", False)  # (an encoder's fragment holds stored blocks of its own: it goes to a byte boundary)
    s.append_bytes(c.compress(text[1000:2600]) + c.flush(zlib.Z_SYNC_FLUSH), text[1000:2600])
    s.fixed_block(False)  # (an empty block: the next fragment's matches reach into this one)
    s.eob()
    s.stored(b"", False)
    s.append_bytes(c.compress(text[2600:4200]) + c.flush(zlib.Z_FULL_FLUSH), text[2600:4200])
    s.fixed_block(True)
    s.lit(0x42)
    s.match(4, 1600)
    s.eob()
    raw, plain, status = s.finish()
    assert status is None and 1500 <= len(raw) <= 3072, len(raw)
    return raw, plain


@functools.lru_cache(maxsize=None)
def small(fmt):
    raw, plain = small_raw()
    return wrap(raw, plain, fmt), plain


@functools.lru_cache(maxsize=1 << 16)
def model_step(state, data, max_out, last, fmt):
    return rm.step(state, data, max_out, last, fmt)


def run(eng, items, fmt=rm.DF_DETECT):
    """items: (state, data, max_out, last) -> the engine's (out, consumed, state, why or None, status) of each"""
    outs, used, states, why, sts = eng.uncompress_resume_batch(
        [d for _, d, _, _ in items], [s for s, _, _, _ in items], [m for _, _, m, _ in items],
        [l for _, _, _, l in items], fmt)
    return [(outs[k], used[k], states[k], why[k] if sts[k] == OK else None, sts[k]) for k in range(len(items))]


def check(eng, items, fmt=rm.DF_DETECT, walks=None):
    """one batch call; every stream's answer is the model's (walks: a rm.Walk a stream, which spares the model the
    blocks it has decoded before)"""
    got = run(eng, items, fmt)
    if walks:  # (thousands of pieces of few streams: nothing of them is worth keeping)
        want = [rm.step(s, bytes(d), m, bool(l), fmt, None, walks[k]) for k, (s, d, m, l) in enumerate(items)]
    else:
        want = [model_step(s, bytes(d), m, bool(l), fmt) for s, d, m, l in items]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, len(items[k][1]), items[k][2:], (len(g[0]), g[1], g[2] and g[2][:64].hex(), g[3:]),
                        (len(w[0]), w[1], w[2] and w[2][:64].hex(), w[3:]))
    return want


# ---- 1. every cut ----
def check_every_cut(eng, fmts=FORMATS, last_stride=1):
    wanted = {"container header", "code-length loop", "stored LEN", "stored data", "trailer"}
    for fmt in fmts:
        z, plain = small(fmt)
        trace, skips = [], set()
        for k in range(len(z) + 1):
            r = rm.step(None, z[:k], BIG, False, rm.DF_DETECT if fmt != rm.DF_DEFLATE else fmt, trace)
            assert r[4] == OK, (fmt, k, r[4])  # no prefix gives an error
            if r[2] is not None:
                skips.add(rm.State(r[2]).bit_skip)
        kinds = {w for w, _ in trace}
        assert skips == set(range(8)), skips
        assert wanted - ({"container header", "trailer"} if fmt == rm.DF_DEFLATE else set()) <= kinds, kinds
        assert kinds & {"length extra bits", "distance extra bits"}
        call_fmt = rm.DF_DETECT if fmt != rm.DF_DEFLATE else fmt
        res = check(eng, [(None, z[:k], BIG, False) for k in range(len(z) + 1)], call_fmt)
        assert res[-1][0] == plain and res[-1][3] == rm.DONE and res[-1][1] == len(z)
        cuts = sorted(set(range(0, len(z) + 1, last_stride)) | {len(z)})
        res = check(eng, [(None, z[:k], BIG, True) for k in cuts], call_fmt)
        assert res[-1][0] == plain and res[-1][3] == rm.DONE
        assert all(r[4] != OK for r in res[:-1]) and any(r[4] == END_OF_BUFFER for r in res)


# ---- 2. chains ----
def check_chain(eng, z, plain, piece, max_out, fmt, garbage=b"\x01\x02\x03\x04\x05\x06\x07"):
    """the stream in pieces, one call a piece (more where the budget stops it); after every call the answer, the state
    included, is the model's"""
    whole = z + garbage
    state, buf, pos, out, calls = None, b"", 0, [], 0
    why = rm.NEED_INPUT
    while why != rm.DONE:
        assert pos < len(whole) or why == rm.NEED_OUTPUT
        if why == rm.NEED_INPUT:
            buf += whole[pos:pos + piece]
            pos += piece
        (o, used, state, why, st), = check(eng, [(state, buf, max_out, False)], fmt)
        assert st == OK
        if why == rm.NEED_OUTPUT and not o:  # a block larger than the budget
            max_out *= 2
        out.append(o)
        buf = buf[used:]
        calls += 1
    assert b"".join(out) == plain and state is None
    assert buf + whole[min(pos, len(whole)):] == garbage  # what stands behind the trailer is left alone
    return calls


def check_chain_small(eng, pieces=(61,)):
    for fmt in FORMATS:
        z, plain = small(fmt)
        for piece in pieces:
            check_chain(eng, z, plain, piece, BIG, rm.DF_DETECT if fmt != rm.DF_DEFLATE else fmt)


def check_chain_mix(eng, configs=((4099, 50000), (70001, BIG))):
    plain = sc.mix()
    for k, (piece, max_out) in enumerate(configs):
        wbits, fmt = sc.WBITS[k % 3]
        z = sc.deflate(plain, 6, wbits, 8)
        calls = check_chain(eng, z, plain, piece, max_out, fmt)
        assert calls > len(z) // piece


# ---- 3. budget ----
def check_budget(eng):
    raw, plain = small_raw()
    _, _, _, _, marks = rm.decode(raw, 0, b"", BIG, False)
    sizes = [marks[k + 1][1] - marks[k][1] for k in range(len(marks) - 1)]
    assert sizes[0] == 300 and sizes[1] == 0 and max(sizes) > 1000
    items = [(None, raw, 300, False), (None, raw, 299, False)]
    # from the third block on: budgets of exactly one block, one below it, and what two and more blocks come to
    first = check(eng, [(None, raw, 300, False)], rm.DF_DEFLATE)[0]
    assert first[0] == plain[:300] and first[3] == rm.NEED_OUTPUT  # the empty stored block and a 1-byte block follow
    st = first[2]
    rest = raw[first[1]:]
    items += [(st, rest, m, False) for m in (1, 2, 8, 9, 10, 300, 339, 340, 341, 631, 632, 5000)]
    # a block in which the budget is passed before the cut, and one in which the cut comes first
    big = max(range(len(sizes)), key=lambda k: sizes[k])
    b0, b1 = marks[big][0] // 8 + 1, (marks[big + 1][0] + 7) // 8
    for cut in (b0 + 40, (b0 + b1) // 2, b1 - 2):
        for m in (marks[big][1] + 10, marks[big][1] + sizes[big] - 1, marks[big][1] + sizes[big]):
            items.append((None, raw[:cut], m, False))
    want = check(eng, items, rm.DF_DEFLATE)
    assert want[1][3] == rm.NEED_OUTPUT and want[1][0] == b"" and want[1][1] == 0
    assert {w[3] for w in want} >= {rm.NEED_INPUT, rm.NEED_OUTPUT}
    assert [w[3] for w in want[-9:]] == [1, 1, 1, 2, 1, 1, 2, 1, 1]  # (the budget is passed before the cut in two of them)
    # two empty blocks at a full budget
    s = dc.Stream()
    s.stored(b"x" * 10, False)
    s.stored(b"", False)
    s.fixed_block(False)
    s.eob()
    s.stored(b"y", True)
    raw2, plain2, _ = s.finish()
    (w,) = check(eng, [(None, raw2, 10, False)], rm.DF_DEFLATE)
    assert w[0] == b"x" * 10 and w[3] == rm.NEED_OUTPUT and rm.State(w[2]).total_in == w[1] == len(raw2) - 6


# ---- 4. the window's edge ----
def check_window_edge(eng):
    filler = sc.mix()[5000:5000 + 32768]
    items = []
    for p in (1, 257, 32767, 32768):
        s = dc.Stream()
        s.stored(filler[:p], False)
        s.fixed_block(True)
        s.match(3, p)
        s.lit(0x21)
        s.eob()
        raw, plain, status = s.finish()
        assert status is None
        (a,) = check(eng, [(None, raw[:p + 5], BIG, False)], rm.DF_DEFLATE)
        assert a[0] == filler[:p] and a[3] == rm.NEED_INPUT and rm.State(a[2]).win_len == p
        items.append((a[2], raw[a[1]:], BIG, True))
        if p == 32768:  # a forged state one byte short: the match reaches beyond the window
            f = rm.State(a[2])
            f.total_out -= 1
            f.win_len -= 1
            f.window = f.window[1:]
            assert rm.sound(f.pack())
            items.append((f.pack(), raw[a[1]:], BIG, True))
    want = check(eng, items, rm.DF_DEFLATE)
    assert [w[4] for w in want] == [OK] * 4 + [INVALID_BUFFER] and all(w[3] == rm.DONE for w in want[:4])


# ---- 5. damage ----
def check_trailers(eng):
    items, want_st = [], []
    for fmt, at, st in ((rm.DF_GZIP, -8, CHECKSUM), (rm.DF_GZIP, -1, SIZE), (rm.DF_ZLIB, -2, CHECKSUM)):
        z, _ = small(fmt)
        bad = bytearray(z)
        bad[at] ^= 0x40
        items += [(None, bytes(bad), BIG, False), (None, bytes(bad), BIG, True)]
        want_st += [st, st]
        # ... in the call that sees the trailer
        (a,) = check(eng, [(None, bytes(bad[:-9]), BIG, False)])
        assert a[4] == OK
        items.append((a[2], bytes(bad[a[1]:]), BIG, False))
        want_st.append(st)
    assert [w[4] for w in check(eng, items)] == want_st


def check_flips(eng, count=64):
    """a flipped byte in the body, the stream in two pieces with `last` on the second: the final status is the whole
    call's"""
    rng = random.Random(17)
    cases = []
    for k in range(count):
        fmt = FORMATS[k % 3]
        z, _ = small(fmt)
        bad = bytearray(z)
        bad[rng.randrange(12, len(z) - 8)] ^= 1 << rng.randrange(8)
        cases.append((fmt, bytes(bad), rng.randrange(1, len(z))))
    whole = []
    for fmt in FORMATS:
        sts = eng.uncompress_batch([c[1] for c in cases if c[0] == fmt], fmt)[1]
        whole += [(k, st) for k, st in zip([k for k, c in enumerate(cases) if c[0] == fmt], sts)]
    whole = dict(whole)
    assert sum(st != OK for st in whole.values()) >= 16
    first = [check(eng, [(None, z[:cut], BIG, False)], fmt)[0] for fmt, z, cut in cases]
    for k, (fmt, z, cut) in enumerate(cases):
        a = first[k]
        if a[4] != OK:  # a definite error surfaced early, with the same code
            assert a[4] == whole[k], (k, a[4], whole[k])
            continue
        (b,) = check(eng, [(a[2], z[a[1]:], BIG, True)], fmt)
        assert b[4] == whole[k], (k, fmt, cut, b[4], whole[k])


def damaged_states(state):
    s = rm.State(state)
    out = []
    for field, value in (("magic", b"ZHRESUM2"), ("version", 2), ("fmt", 0), ("fmt", 4), ("phase", 0), ("phase", 3),
                         ("bit_skip", 8), ("win_len", s.win_len + 1), ("win_len", s.win_len - 1),
                         ("total_out", s.total_out + 70000), ("reserved", b"\1" + bytes(15)),
                         ("reserved", bytes(15) + b"\1")):
        d = rm.State(state)
        setattr(d, field, value)
        out.append(d.pack())
    d = rm.State(state)
    d.phase, d.bit_skip = 2, 3
    out += [d.pack(), state + b"\0", state[:-1], state[:63], b""]
    assert not any(rm.sound(b) for b in out)
    return out


def check_static_damage(eng):
    z, plain = small(rm.DF_GZIP)
    (a,) = check(eng, [(None, z[:1500], BIG, False)])
    assert a[4] == OK and rm.sound(a[2]) and rm.State(a[2]).win_len > 1
    bad = damaged_states(a[2])
    want = check(eng, [(b, z[a[1]:], BIG, False) for b in bad] + [(a[2], z[a[1]:], BIG, False)])
    assert [w[4] for w in want] == [INVALID_BUFFER] * len(bad) + [OK] and want[-1][3] == rm.DONE


def check_batch33(eng):
    """new streams, resumed streams, bad states and bad bytes side by side: nobody's answer depends on a neighbour's"""
    z, plain = small(rm.DF_ZLIB)
    rng = random.Random(3)
    (a,) = check(eng, [(None, z[:1200], BIG, False)])
    bad_state = damaged_states(a[2])[7]
    hurt = bytearray(z)
    hurt[400] ^= 0xff
    items = []
    for k in range(33):
        kind = k % 4
        if kind == 0:
            items.append((None, z[:rng.randrange(len(z) + 1)], rng.choice((100, 700, BIG)), False))
        elif kind == 1:
            items.append((a[2], z[a[1]:a[1] + rng.randrange(len(z))], rng.choice((700, BIG)), bool(k & 4)))
        elif kind == 2:
            items.append((bad_state, z[a[1]:], BIG, False))
        else:
            items.append((None, bytes(hurt), BIG, bool(k & 4)))
    want = check(eng, items)
    assert len({w[4] for w in want}) >= 3 and {w[3] for w in want} >= {rm.DONE, rm.NEED_INPUT, rm.NEED_OUTPUT, None}
    alone = [check(eng, [it])[0] for it in items[:8]]
    assert alone == want[:8]


# ---- 6. hand-built streams ----
def spread(cuts, marks, cap):
    """at most about `cap` of a stream's cuts: the first and the last two, the middle byte (it is among them), the first
    boundary of every bit residue, and the rest evenly"""
    if len(cuts) <= cap:
        return cuts
    keep = set(cuts[:2] + cuts[-2:] + [cuts[len(cuts) // 2]])
    for r in range(8):
        keep |= {b // 8 for b in [b for b, _ in marks[1:] if b % 8 == r][:1]}
    keep |= set(cuts[::max(1, len(cuts) // max(1, cap - len(keep)))])
    return sorted(keep & set(cuts))


@functools.lru_cache(maxsize=None)
def crafted_walks(small_set):
    return [rm.Walk(c[1]) for c in sc.parity_crafted(small_set)]


def check_crafted(eng, small_set=False, cap=None):
    """every hand-built stream of tests/parity_cases.py cut at its middle byte and at the byte that holds each of its
    block boundaries, in two calls; what the whole call rejects ends with the whole call's status.  cap (the
    emulator's): of a stream with more cuts than that, a spread() of them."""
    cases = sc.parity_crafted(small_set)
    walks = crafted_walks(small_set)
    whole = eng.uncompress_batch([c[1] for c in cases], rm.DF_DEFLATE)[1]
    n_cuts = n_bad = 0
    group, group_bytes = [], 0
    for k, (name, raw, plain, _) in enumerate(cases):
        marks = list(zip(walks[k].bits, walks[k].outs))
        cuts = sorted({len(raw) // 2} | {min(len(raw), b // 8) for b, _ in marks[1:]})
        for cut in (spread(cuts, marks, cap) if cap else cuts):
            group.append((k, cut))
            group_bytes += cut
            if group_bytes > (48 << 20):  # (batches of about 48 MiB of input: the cuts of one stream may take several)
                n_bad += crafted_group(eng, cases, walks, whole, group)
                n_cuts += len(group)
                group, group_bytes = [], 0
    n_bad += crafted_group(eng, cases, walks, whole, group)
    n_cuts += len(group)
    assert n_bad > 20
    if not cap and not small_set:
        assert n_cuts > 30000  # (every cut: a dozen of the streams have hundreds or thousands of blocks)


def crafted_group(eng, cases, walks, whole, owner):
    """the two calls of the cuts `owner` [(stream, cut)] -> how many of them the whole call rejects"""
    firsts = [(None, cases[k][1][:cut], 1 << 30, False) for k, cut in owner]
    a = check(eng, firsts, rm.DF_DEFLATE, [walks[k] for k, _ in owner])
    seconds, idx = [], []
    for j, (k, cut) in enumerate(owner):
        name, raw, plain, _ = cases[k]
        if a[j][4] != OK:
            assert a[j][4] == whole[k], (name, cut, a[j][4], whole[k])
            continue
        if a[j][2] is None:  # (done already: a final block before the cut)
            assert whole[k] == OK and a[j][3] == rm.DONE, name
            continue
        seconds.append((a[j][2], raw[a[j][1]:], 1 << 30, True))
        idx.append(j)
    b = check(eng, seconds, rm.DF_DEFLATE, [walks[owner[j][0]] for j in idx])
    n_bad = 0
    for j, r in zip(idx, b):
        k, cut = owner[j]
        name, raw, plain, _ = cases[k]
        if whole[k] != OK:
            n_bad += 1
            assert r[4] == whole[k], (name, cut, r[4], whole[k])
        else:
            assert r[4] == OK and r[3] == rm.DONE and a[j][0] + r[0] == plain, (name, cut)
    return n_bad


# ---- 7. members ----
def check_members(eng):
    z, plain = small(rm.DF_GZIP)
    z2 = wrap(zlib.compress(plain[::-1], 9)[2:-4], plain[::-1], rm.DF_GZIP, b"")
    (a,) = check(eng, [(None, z + z2, BIG, False)])
    assert a[0] == plain and a[3] == rm.DONE and a[1] == len(z) and a[2] is None
    (b,) = check(eng, [(None, (z + z2)[a[1]:], BIG, True)])
    assert b[0] == plain[::-1] and b[3] == rm.DONE and b[1] == len(z2)


# ---- 8. call errors ----
def check_call_errors(eng):
    import ctypes as c
    lib, h = eng.lib, eng._h
    z, _ = small(rm.DF_ZLIB)
    src = (c.c_void_p * 1)(c.cast(c.c_char_p(z), c.c_void_p))
    ln = (c.c_size_t * 1)(len(z))
    mo = (c.c_uint64 * 1)(BIG)
    zero = (c.c_uint64 * 1)(0)
    out, olen, used = (c.c_void_p * 1)(), (c.c_size_t * 1)(), (c.c_size_t * 1)()
    ns, nsl, why, st = (c.c_void_p * 1)(), (c.c_size_t * 1)(), (c.c_int32 * 1)(), (c.c_int32 * 1)(5)
    f = lib.zh_uncompress_resume_batch
    assert f(h, None, None, 0, 0, None, None, None, None, None, None, None, None, None, None, None) == 0  # n == 0
    args = [src, ln, 1, 0, None, None, mo, None, out, olen, used, ns, nsl, why, st]
    for k in (0, 1, 6, 8, 9, 10, 11, 12, 13, 14):
        broken = list(args)
        broken[k] = None
        assert f(h, *broken) == ARGUMENT, k
    assert f(h, *(args[:6] + [zero] + args[7:])) == ARGUMENT             # max_out == 0
    assert f(h, *(args[:4] + [None, ln] + args[6:])) == ARGUMENT         # state_lens without states
    null = (c.c_void_p * 1)()
    assert f(h, *([null] + args[1:])) == ARGUMENT                        # a NULL source with a length
    assert f(h, *(args[:3] + [9] + args[4:])) == 2 and st[0] == 2        # a bad format: the call's and every stream's
    assert f(h, *args) == 0 and st[0] == 0 and why[0] == rm.DONE and used[0] == len(z)
    lib.zh_free(out[0])


# ---- the dumped cases of tests/resume_main.cpp ----
class Recorder:
    """an engine that answers with the model and keeps every call"""

    def __init__(self):
        self.calls = []

    def uncompress_resume_batch(self, srcs, states, max_out, last, fmt):
        res = [model_step(s, bytes(d), m, bool(l), fmt) for s, d, m, l in zip(states, srcs, max_out, last)]
        self.calls.append((fmt, list(zip(states, srcs, max_out, last)), res))
        return ([r[0] for r in res], [r[1] for r in res], [r[2] for r in res], [r[3] if r[3] is not None else 0 for r in res],
                [r[4] for r in res])


def dump(path):
    """Cases 1 (one container, `last` on every seventh prefix), 3, 4 and 5 (without the flips, which need the whole
    call's statuses) as one file of calls: u32 calls; a call: u32 streams, u32 format; a stream: state (u64 length,
    all ones: none; bytes), input (u64, bytes), u64 max_out, u8 last, then what the model answers: i32 status, i32 why
    (-1: none), u64 consumed, output (u64, bytes), state (as above).  -> (calls, streams)"""
    rec = Recorder()
    check_every_cut(rec, (rm.DF_ZLIB,), last_stride=7)
    check_budget(rec)
    check_window_edge(rec)
    check_trailers(rec)
    check_static_damage(rec)
    check_batch33(rec)
    none = struct.pack("<Q", (1 << 64) - 1)
    blob = lambda b: none if b is None else struct.pack("<Q", len(b)) + bytes(b)
    out = [struct.pack("<I", len(rec.calls))]
    for fmt, items, res in rec.calls:
        out.append(struct.pack("<II", len(items), fmt))
        for (state, data, max_out, last), (o, used, nstate, why, st) in zip(items, res):
            out += [blob(state), blob(data), struct.pack("<QB", max_out, 1 if last else 0),
                    struct.pack("<iiQ", st, -1 if why is None else why, used), blob(o), blob(nstate)]
    with open(path, "wb") as f:
        f.write(b"".join(out))
    return len(rec.calls), sum(len(c[1]) for c in rec.calls)
