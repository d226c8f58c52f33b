"""Cases of zh_compress_stream_batch shared by tests/test_emu_stream.py (fiber emulator), tests/test_gpu_stream.py
(MI355X) and, through ModelEngine and dump(), the sanitized program of tests/test_stream_sanitize.py.  Every answer --
output, new state, status -- is held byte for byte against the model's (tests/stream_model.py); every family asserts
from the model's records that it reaches what it is there for, before the engine runs."""
import functools
import random
import struct
import zlib

import oracle
import stream_model as sm

OK, INVALID_BUFFER, ARGUMENT = 0, 13, 22
BLOCK, SYNC, FINISH = sm.BLOCK, sm.SYNC, sm.FINISH
FORMATS = (sm.DF_DEFLATE, sm.DF_ZLIB, sm.DF_GZIP)
WBITS = {sm.DF_DEFLATE: -15, sm.DF_ZLIB: 15, sm.DF_GZIP: 31}
LENGTHS = (0, 1, 14, 15, 32767, 32768, 32769, 65535, 65536, 65537)
LEVELS = (-2, 0, 1, 2, 6, 9)
WORDS = [w.encode() for w in ("stream", "block", "flush", "the", "of", "a", "deflate", "window", "piece", "bits",
                              "pending", "stored", "marker", "byte", "and", "gzip", "sync", "finish", "wave", "lane")]


@functools.lru_cache(maxsize=None)
def text(n, seed=0):
    rng = random.Random(1000 + seed)
    out = bytearray()
    while len(out) < n:
        out += rng.choice(WORDS) + rng.choice((b" ", b" ", b", ", b".\n"))
    return bytes(out[:n])


@functools.lru_cache(maxsize=None)
def rnd(n, seed=0):
    return random.Random(2000 + seed).randbytes(n)


class Chain:
    """one stream's life: pieces[j] fed with flushes[j]"""

    def __init__(self, pieces, flushes, level, fmt, block_bytes=32768):
        assert len(pieces) == len(flushes)
        self.pieces, self.flushes, self.level, self.fmt, self.bb = list(pieces), list(flushes), level, fmt, block_bytes
        self.records = []

    @property
    def whole(self):
        return b"".join(self.pieces)


def call(eng, items, level, fmt, bb):
    """one batch call of (state, piece, flush) items -> [(output, state, status)]"""
    outs, states, sts = eng.compress_stream_batch([p for _, p, _ in items], [s for s, _, _ in items],
                                                  [f for _, _, f in items], level, fmt, bb)
    return list(zip(outs, states, sts))


def run_chains(eng, chains, fname_len=0):
    """All chains side by side: call j feeds piece j of every chain that has one.  New streams of one (level, format,
    block size) share a call; resumed streams of every kind share one, whose own level, format and block size are
    nonsense -- a resumed stream takes them from its state.  Every answer is the model's.  -> the streams"""
    n = len(chains)
    states, acc = [None] * n, [b""] * n
    for j in range(max(len(c.pieces) for c in chains)):
        idx = [c for c in range(n) if j < len(chains[c].pieces)]
        groups = {}
        for c in idx:
            groups.setdefault((chains[c].level, chains[c].fmt, chains[c].bb) if j == 0 else None, []).append(c)
        for key, grp in groups.items():
            items = [(states[c], chains[c].pieces[j], chains[c].flushes[j]) for c in grp]
            got = call(eng, items, *(key if key else (99, 0, 7)))
            for c, g in zip(grp, got):
                ch = chains[c]
                want = sm.step(states[c], ch.pieces[j], ch.flushes[j], ch.level, ch.fmt, ch.bb, fname_len, ch.records)
                assert g == want, (c, j, len(ch.pieces[j]), ch.flushes[j], ch.level, ch.fmt, ch.records[-1],
                                   (len(g[0]), g[0][:24].hex(), g[0][-24:].hex(), g[1] and g[1].hex(), g[2]),
                                   (len(want[0]), want[0][:24].hex(), want[0][-24:].hex(), want[1] and want[1].hex(), want[2]))
                states[c] = want[1]
                acc[c] += want[0]
    return acc


def decodes(stream, fmt, plain, finished=True):
    d = zlib.decompressobj(WBITS[fmt])
    got = d.decompress(stream)
    assert got == plain, (len(got), len(plain))
    if finished:
        assert d.eof and not d.unused_data
        assert oracle.uncompress(stream, fmt) == plain


def check_chains(eng, chains, fname_len=0):
    streams = run_chains(eng, chains, fname_len)
    for ch, z in zip(chains, streams):
        if ch.flushes[-1] == FINISH:
            decodes(z, ch.fmt, ch.whole)
        elif ch.flushes[-1] == SYNC:
            decodes(z, ch.fmt, ch.whole, finished=False)
    return streams


# ---- 1. the alignment family ----
ALIGN_N = 100  # (with 40 the model misses k = 1, 3, 5 and 7: test_stream_model.py)


@functools.lru_cache(maxsize=None)
def short(n):
    """n bytes of very repetitive text: the oracle codes it (a fixed block with matches) from a dozen bytes on, and the
    bits it takes, hence the pending bits behind it, change every few bytes"""
    rng = random.Random(77)
    out = bytearray()
    while len(out) < n:
        out += rng.choice((b"ab", b"ba", b"a a", b"b"))
    return bytes(out[:n])


def big_piece(seed):
    return text(32768, seed) + rnd(32768, seed) + text(100, seed + 1)


def align_chains(fmts, levels=(1, 6), ns=None):
    """per short piece of n bytes and level: the short piece with BLOCK, then text(32768) + random(32768) + text(100) --
    a coded block, a stored one, a coded one -- behind the bits it left, with BLOCK and with SYNC"""
    chains = []
    for q, n in enumerate(ns or range(1, ALIGN_N + 1)):
        for level in levels:
            fmt = fmts[(q + level) % len(fmts)]
            chains.append(Chain([short(n), big_piece(n), b""], [BLOCK, BLOCK, FINISH], level, fmt))
            chains.append(Chain([short(n), big_piece(n), short(n), b"end"], [BLOCK, SYNC, SYNC, FINISH], level, fmt))
    return chains


def align_tags(chains):
    """what a family reaches: the pending bits k its big pieces were placed behind, the byte delta and (p + 3) mod 8 of
    their stored block, the bits left pending behind them, the residue in front of a marker"""
    tags = set()
    for ch in chains:
        r = ch.records[1]
        tags |= {("k", r["k"]), ("delta", r["delta"]), ("p3", r["p3"])}
        if ch.flushes[1] == BLOCK:
            tags.add(("pend", r["pend"]))
        tags |= {("residue", r["residue"]) for r in ch.records if "residue" in r}
    return tags


ALIGN_ALL = ({("delta", 0), ("delta", 1)}
             | {(what, v) for what in ("k", "p3", "pend", "residue") for v in range(8)})


@functools.lru_cache(maxsize=None)
def align_cover():
    """a few n whose chains reach, between them, all the full family reaches (the emulator's family)"""
    per_n = {}
    for n in range(1, ALIGN_N + 1):
        chains = align_chains((sm.DF_DEFLATE,), ns=(n,))
        run_chains(ModelEngine(), chains)
        per_n[n] = align_tags(chains)
    left, ns = set(ALIGN_ALL), []
    while left:
        n = max(per_n, key=lambda m: len(per_n[m] & left))
        assert per_n[n] & left, left  # (the full family reaches everything)
        ns.append(n)
        left -= per_n[n]
    return tuple(sorted(ns))


def check_align(eng, fmts=FORMATS, thin=False):
    """thin: the covering few of align_cover(), the formats taking turns; else the whole family in every format"""
    for one in ([tuple(fmts)] if thin else [(f,) for f in fmts]):
        chains = align_chains(one, ns=align_cover() if thin else None)
        check_chains(eng, chains)
        assert align_tags(chains) == ALIGN_ALL, ALIGN_ALL - align_tags(chains)


# ---- 2. piece lengths ----
def length_chains(levels, fmts, lengths=LENGTHS):
    chains = []
    data = text(40000, 3) + rnd(9000, 3) + text(20000, 4)
    for q, level in enumerate(levels):
        for fmt in fmts:
            for L in lengths:
                for fl in (BLOCK, SYNC, FINISH):
                    if fl == FINISH:
                        chains.append(Chain([data[:L]], [FINISH], level, fmt))
                    else:
                        chains.append(Chain([data[:L], b"xyz"], [fl, FINISH], level, fmt))
    return chains


def check_lengths(eng, levels=LEVELS, fmts=FORMATS, lengths=LENGTHS):
    check_chains(eng, length_chains(levels, fmts, lengths))


# ---- 3. stored blocks ----
def stored_chains(fmts=FORMATS):
    chains = []
    for fmt in fmts:
        for fl in (BLOCK, SYNC, FINISH):
            tail = ([], []) if fl == FINISH else ([text(50, 1)], [FINISH])
            mk = lambda piece, level, bb=32768: Chain([short(30), piece] + tail[0], [BLOCK, fl] + tail[1], level, fmt, bb)
            chains.append(mk(text(150000, 2) + rnd(50000, 2), 0))                # several stored chunks in one piece
            chains.append(mk(rnd(140000, 3), 1, 131072))                        # a stored block longer than 65535 bytes
            chains.append(mk(rnd(32768, 4) + text(32768, 4), 1))                 # stored first
            chains.append(mk(text(32768, 5) + rnd(32768, 5), 1))                 # stored last
            chains.append(mk(rnd(1000, 6), 1))                                   # stored only
            chains.append(mk(rnd(32768, 7) + text(32768, 7) + rnd(40000, 8), 6))  # two stored blocks, a coded one between
    return chains


def check_stored(eng, fmts=FORMATS):
    chains = stored_chains(fmts)
    check_chains(eng, chains)
    for ch in chains:
        assert "p3" in ch.records[1], ch.records  # (the premise: the piece's stream has a stored block)
    assert any(ch.records[1]["k"] for ch in chains)


# ---- 4. empty pieces ----
def empty_chains(fmts=FORMATS, level=1):
    chains = []
    for fmt in fmts:
        t = text(700, 9)
        chains.append(Chain([t, b""], [BLOCK, FINISH], level, fmt))             # FINISH alone behind pending bits
        chains.append(Chain([t, b""], [SYNC, FINISH], level, fmt))
        chains.append(Chain([b""], [FINISH], level, fmt))                       # ... and as the only call
        chains.append(Chain([b"", t, b"", b"", t], [BLOCK, BLOCK, BLOCK, SYNC, FINISH], level, fmt))  # no-ops, a bare marker
        chains.append(Chain([b"", b"", t, b""], [SYNC, SYNC, BLOCK, FINISH], level, fmt))
        chains.append(Chain([b"", b""], [BLOCK, FINISH], 0, fmt))
    return chains


def check_empty(eng, fmts=FORMATS):
    chains = empty_chains(fmts)
    check_chains(eng, chains)
    assert any(ch.records[-1]["k"] for ch in chains)  # an empty FINISH placed behind pending bits


# ---- 5. identity ----
def check_identity(eng, fmts=FORMATS, levels=(1, 6, 0)):
    whole = text(50000, 11) + rnd(40000, 11) + text(80000, 12) + b"tail"
    chains = []
    for level in levels:
        unit = 65535 if level == 0 else 32768
        cuts, at, rng = [], 0, random.Random(level)
        while at < len(whole):
            step = unit * rng.randint(1, 3)
            cuts.append(whole[at:at + step])
            at += step
        assert len(cuts) >= 2 and len(cuts[0]) % unit == 0
        for fmt in fmts:
            chains.append(Chain(cuts, [BLOCK] * (len(cuts) - 1) + [FINISH], level, fmt))
    for ch, z in zip(chains, check_chains(eng, chains)):
        assert z == oracle.compress_blocks(whole, ch.level, ch.fmt, 32768)[0], (ch.level, ch.fmt)


# ---- 6. a batch of streams at different points of their lives ----
def batch33(eng, call_fn=None):
    """-> (items, level, fmt, bb, wanted answers): 33 streams in one call -- new ones, streams resumed with every k,
    finishing ones, ones whose state is damaged -- with the states made by the model"""
    fmt, level, bb = sm.DF_GZIP, 1, 32768
    items = []
    by_k = {}
    for n in range(1, 200):
        out, st, _ = sm.step(None, short(n), BLOCK, level, fmt, bb)
        by_k.setdefault(sm.State(st).pend_bits, st)
        if len(by_k) == 8:
            break
    assert sorted(by_k) == list(range(8))
    for k in range(8):
        items.append((by_k[k], big_piece(k), (BLOCK, SYNC, FINISH)[k % 3]))
        items.append((by_k[k], text(900 + k, k), (SYNC, FINISH, BLOCK)[k % 3]))
    for j in range(6):
        items.append((None, text(5000 * j, j) + rnd(300 * j, j), (BLOCK, SYNC, FINISH)[j % 3]))
    other = sm.step(None, text(77, 1), BLOCK, 6, sm.DF_ZLIB, 65536)[1]  # a stream of another level, format, block size
    items.append((other, text(70000, 2), SYNC))
    items.append((other, b"", FINISH))
    bad = bytearray(by_k[3])
    bad[0] ^= 1
    items.append((bytes(bad), text(100, 1), SYNC))
    items.append((by_k[5][:63], text(100, 1), SYNC))
    items.append((by_k[2], b"", BLOCK))
    items.append((by_k[6], b"", SYNC))
    items.append((None, b"", BLOCK))
    while len(items) < 33:
        items.append((by_k[len(items) % 8], rnd(40000, len(items)), FINISH))
    assert len(items) == 33
    want = [sm.step(s, p, f, level, fmt, bb) for s, p, f in items]
    assert sum(w[2] != OK for w in want) == 2
    return items, level, fmt, bb, want


def check_batch33(eng):
    items, level, fmt, bb, want = batch33(eng)
    assert call(eng, items, level, fmt, bb) == want
    for k, it in enumerate(items):  # ... and one by one
        assert call(eng, [it], level, fmt, bb) == [want[k]], k


# ---- 7. bad states, argument errors ----
def bad_states():
    good = sm.step(None, short(30), BLOCK, 1, sm.DF_GZIP, 32768)[1]
    s = sm.State(good)
    assert s.pend_bits and s.pend_bits < 7
    mk = lambda **kw: sm.pack_state(**{**dict(fmt=s.fmt, level=s.level, block_bytes=s.block_bytes, pend_bits=s.pend_bits,
                                              pend_byte=s.pend_byte, check=s.check, total_in=s.total_in,
                                              total_out=s.total_out), **kw})
    assert mk() == good
    return good, [mk(magic=b"ZHCSTRM2"), mk(version=2), mk(fmt=0), mk(fmt=4), mk(level=-3), mk(level=10),
                  mk(block_bytes=0), mk(block_bytes=32769), mk(block_bytes=16384), mk(block_bytes=8388608), mk(phase=0),
                  mk(phase=2), mk(pend_bits=8), mk(pend_byte=1 << s.pend_bits), mk(pend_byte=0x100), mk(reserved=1),
                  good[:63], good + b"\0", b""]


def check_bad_states(eng):
    good, bads = bad_states()
    piece = text(3000, 2)
    items = []
    for b in bads:
        items += [(good, piece, SYNC), (b, piece, SYNC)]
    items.append((None, piece, FINISH))
    got = call(eng, items, 1, sm.DF_GZIP, 32768)
    want = [sm.step(s, p, f, 1, sm.DF_GZIP, 32768) for s, p, f in items]
    assert got == want
    assert [g[2] for g in got] == [OK, INVALID_BUFFER] * len(bads) + [OK]
    assert all(g[0] == b"" and g[1] is None for g in got[1::2])  # nothing from a failed stream; its neighbours whole


def check_call_errors(eng):
    from zippy_amd.common import ZippyError
    good, _ = bad_states()

    def refused(items, level=1, fmt=sm.DF_GZIP, bb=32768):
        try:
            call(eng, items, level, fmt, bb)
        except ZippyError as e:
            return e.status
        return OK
    new, old = (None, b"abc", SYNC), (good, b"abc", SYNC)
    assert refused([new]) == OK and refused([old]) == OK
    for kw in (dict(level=10), dict(level=-3), dict(fmt=0), dict(fmt=4), dict(bb=1), dict(bb=32769), dict(bb=8388608)):
        assert refused([old, new], **kw) == ARGUMENT, kw
        assert refused([old], **kw) == OK, kw  # (nothing new: nothing of the call's own is looked at)
    assert refused([(None, b"abc", 3)]) == ARGUMENT and refused([old, (good, b"", 255)]) == ARGUMENT
    assert eng.compress_stream_batch([], None, None, 1, sm.DF_GZIP, 0) == ([], [], [])
    # the errors the binding cannot make, at the C boundary with a live context: each is ZH_ERR_ARGUMENT for the call,
    # nothing is handed out, and the good call behind them works
    import ctypes as c
    lib, h = eng.lib, eng._h
    piece = b"abcabcabc"
    src = (c.c_void_p * 1)(c.cast(c.c_char_p(piece), c.c_void_p))
    ln = (c.c_size_t * 1)(len(piece))
    sp = (c.c_void_p * 1)(c.cast(c.c_char_p(good), c.c_void_p))
    sl = (c.c_size_t * 1)(len(good))
    fl = (c.c_uint8 * 1)(SYNC)
    null = (c.c_void_p * 1)()
    out, olen, ns, nsl, st = (c.c_void_p * 1)(), (c.c_size_t * 1)(), (c.c_void_p * 1)(), (c.c_size_t * 1)(), (c.c_int32 * 1)()
    f = lib.zh_compress_stream_batch
    assert f(h, None, None, 0, 1, sm.DF_GZIP, 32768, None, None, None, None, None, None, None, None) == OK  # n == 0
    args = [src, ln, 1, 1, sm.DF_GZIP, 32768, sp, sl, fl, out, olen, ns, nsl, st]

    def refused_raw(a, what):
        assert f(h, *a) == ARGUMENT, what
        assert out[0] is None and ns[0] is None and olen[0] == 0 and nsl[0] == 0, what
    for k in (0, 1, 9, 10, 11, 12, 13):  # every array a call cannot do without
        refused_raw(args[:k] + [None] + args[k + 1:], k)
    refused_raw([null] + args[1:], "a NULL source with a length")
    refused_raw(args[:6] + [None, sl] + args[8:], "state_lens without states")
    refused_raw(args[:6] + [sp, None] + args[8:], "states without state_lens")
    refused_raw(args[:6] + [null, sl] + args[8:], "a NULL state with a length")
    for a, state in ((args, good), (args[:6] + [None, None, None] + args[9:], None)):  # (flush NULL: all SYNC)
        assert f(h, *a) == OK and st[0] == OK
        want = sm.step(state, piece, SYNC, 1, sm.DF_GZIP, 32768)
        assert c.string_at(out[0], olen[0]) == want[0] and c.string_at(ns[0], nsl[0]) == want[1]
        lib.zh_free(out[0])
        lib.zh_free(ns[0])
        out[0] = ns[0] = None
        olen[0] = nsl[0] = 0


# ---- 9. contract mode ----
def check_contract_mode(eng):
    eng.set_l1_parse(1)
    try:
        for fmt in FORMATS:
            pieces = [text(5, 1), text(70000, 3) + rnd(2000, 3), b"", text(33000, 4), rnd(100, 5)]
            flushes = [BLOCK, SYNC, BLOCK, BLOCK, FINISH]
            state, z = None, b""
            for p, f in zip(pieces, flushes):
                ((out, state, st),) = call(eng, [(state, p, f)], 1, fmt, 32768)
                assert st == OK
                z += out
            assert state is None
            decodes(z, fmt, b"".join(pieces))
    finally:
        eng.set_l1_parse(-1)


# ---- the default block size: the reference's own bytes (GPU only: 9 MiB at level 1) ----
def check_default_block(eng):
    whole = (text(3 << 20, 31) + rnd(1 << 20, 31) + text(5 << 20, 32) + rnd(123, 33))
    assert len(whole) == (9 << 20) + 123
    state, z = None, b""
    for at in range(0, len(whole), 4 << 20):
        piece = whole[at:at + (4 << 20)]
        ((out, state, st),) = call(eng, [(state, piece, FINISH if at + len(piece) == len(whole) else BLOCK)], 1,
                                   sm.DF_GZIP, 0)
        assert st == OK
        z += out
    assert state is None and z == oracle.compress(whole, 1, sm.DF_GZIP, 0)


# ---- the sanitized program's cases ----
class ModelEngine:
    """an engine whose answers are the model's and that keeps every call: the cases above, run on it, are what
    tests/stream_main.cpp replays"""

    def __init__(self):
        self.calls = []

    def compress_stream_batch(self, srcs, states=None, flush=None, level=-1, dataFormat=sm.DF_GZIP, block_bytes=0):
        n = len(srcs)
        states = states if states is not None else [None] * n
        flush = flush if flush is not None else [SYNC] * n
        want = [sm.step(states[k], srcs[k], flush[k], level, dataFormat, block_bytes) for k in range(n)]
        self.calls.append((level, dataFormat, block_bytes, list(zip(states, srcs, flush)), want))
        return [w[0] for w in want], [w[1] for w in want], [w[2] for w in want]


def dump(path):
    """u32 calls; a call: u32 streams, i32 level, u32 format, u64 block_bytes; a stream: state (u64 length, all ones:
    none; bytes), piece (u64, bytes), u8 flush, then the model's answer: i32 status, output (u64, bytes), state (as
    above) -> (calls, streams)"""
    eng = ModelEngine()
    check_align(eng, (sm.DF_GZIP, sm.DF_DEFLATE), thin=True)
    check_stored(eng, (sm.DF_ZLIB,))
    check_empty(eng)
    check_lengths(eng, (1, 0), (sm.DF_GZIP,), (0, 1, 15, 32769))
    check_bad_states(eng)
    check_batch33(eng)

    def blob(b):
        return struct.pack("<Q", (1 << 64) - 1) if b is None else struct.pack("<Q", len(b)) + bytes(b)
    streams = 0
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(eng.calls)))
        for level, fmt, bb, items, want in eng.calls:
            fh.write(struct.pack("<IiIQ", len(items), level, fmt, bb))
            for (state, piece, fl), (out, new, st) in zip(items, want):
                fh.write(blob(state) + blob(piece) + struct.pack("<B", fl) + struct.pack("<i", st) + blob(out) + blob(new))
                streams += 1
    return len(eng.calls), streams
