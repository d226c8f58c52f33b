"""Cases of zh_uncompress_ranges / zh_plan_uncompress_ranges shared by tests/test_emu_ranges.py (fiber emulator) and
tests/test_gpu_ranges.py (MI355X).  The expected bytes of a range are always the slice src[off:off + len] of the
original input.  `make(src, level, fmt, block_bytes)` returns (stream, index): oracle.compress_blocks under the
emulator, the engine's own compress_blocks on the GPU (existing tests hold the two equal)."""
import ctypes as c
import random

import numpy as np

import deflate_craft as dc
import oracle
import synth

OK, INVALID_BUFFER, DST_TOO_SMALL, ARGUMENT = 0, 13, 21, 22
BB = 32768
M64 = (1 << 64) - 1


def make_oracle(src, level, fmt, bb):
    return oracle.compress_blocks(src, level, fmt, bb, fname_len=0)


def make_engine(eng):
    return lambda src, level, fmt, bb: eng.compress_blocks(src, level, fmt, bb)


_MIX = {}


def mix(size, index=0):
    """`size` bytes of the G-mix (text, binaries, runs), made once"""
    if (size, index) not in _MIX:
        _MIX[size, index] = synth.gen_mix_buffer(index, size).tobytes()
    return _MIX[size, index]


def pattern(size):
    """no two neighbours alike (a copy one byte off shows in a range of one byte), long matches (a decode the emulator
    gets through quickly)"""
    return bytes((7 * i + 13 * (i // 251)) & 0xff for i in range(size))


def want_slice(src, off, length):
    return src[off:off + length] if off < len(src) else b""


def check_call(eng, srcs, streams, indexes, ranges, bad=()):
    """One host call: every range not in `bad` returns its slice with status 0.  -> (outs, statuses)"""
    outs, sts = eng.uncompress_ranges(streams, indexes, ranges)
    assert len(outs) == len(sts) == len(ranges)
    for r, (s, off, length) in enumerate(ranges):
        if r in bad:
            continue
        assert sts[r] == OK, (r, ranges[r], sts[r])
        assert outs[r] == want_slice(srcs[s], off, length), (r, ranges[r])
    return outs, sts


# ---- the device form ----
class DeviceBuf:
    def __init__(self, eng, data):
        self.eng, self.n = eng, len(data)
        p = c.c_void_p()
        eng._check(eng.lib.zh_device_malloc(eng._h, max(256, len(data)), c.byref(p)))
        self.p = p
        self.write(data)

    def write(self, data):
        if len(data):
            self.eng._check(self.eng.lib.zh_device_upload(self.eng._h, self.p, bytes(data), len(data)))

    def read(self):
        out = (c.c_char * max(1, self.n))()
        if self.n:
            self.eng._check(self.eng.lib.zh_device_download(self.eng._h, out, self.p, self.n))
        return out.raw[:self.n]

    def free(self):
        self.eng.lib.zh_device_free(self.eng._h, self.p)


def pack_streams(streams):
    """-> (image, src_off, src_len): the streams at 256-byte steps, three odd bytes in front of each"""
    img, off, ln = bytearray(), [], []
    for k, s in enumerate(streams):
        img += b"\xee" * ((-len(img)) % 256 + (k % 4))
        off.append(len(img))
        ln.append(len(s))
        img += s
    return bytes(img) + b"\xee" * 16, off, ln


def run_plan(eng, srcs, streams, indexes, ranges, dst_off, dst_cap, dst_size, runs=1):
    """The device plan over `ranges` into slots of a 0xA5-filled destination, run `runs` times (the destination poisoned
    again in between; every run must give what the first gave).  Checks statuses and lengths against the slices, and
    EVERY byte of the destination: a slot's slice where the range succeeded, 0xA5 everywhere else -- but for the
    clipped length of a range that failed on a block, whose slot is unspecified.  -> (lengths, statuses, stats)"""
    img, soff, slen = pack_streams(streams)
    d_src, d_dst = DeviceBuf(eng, img), DeviceBuf(eng, b"\xa5" * dst_size)
    plan = eng.plan_uncompress_ranges(soff, slen, indexes, ranges, dst_off, dst_cap)
    try:
        first = None
        for run in range(runs):
            if run:
                d_dst.write(b"\xa5" * dst_size)
            plan.run(d_src.p, d_dst.p)
            lens, sts = plan.results()
            stats = eng.debug_range_stats()
            got = d_dst.read()
            if first is None:
                first = (lens, sts, got)
            assert (lens, sts, got) == first, "run %d differs from the first" % run
        want = np.full(dst_size, 0xA5, np.uint8)
        loose = np.zeros(dst_size, bool)
        for r, (s, off, length) in enumerate(ranges):
            w = want_slice(srcs[s], off, length)
            if sts[r] == OK:
                assert lens[r] == len(w), (r, ranges[r], lens[r])
                want[dst_off[r]:dst_off[r] + len(w)] = np.frombuffer(w, np.uint8)
            elif sts[r] != DST_TOO_SMALL:  # (a slot too small is not written at all)
                assert lens[r] == 0
                loose[dst_off[r]:dst_off[r] + len(w)] = True
        g = np.frombuffer(got, np.uint8)
        diff = np.flatnonzero((g != want) & ~loose)
        assert diff.size == 0, "destination byte %d (of %d wrong)" % (diff[0], diff.size)
        return lens, sts, stats
    finally:
        plan.close()
        d_src.free()
        d_dst.free()


def slots_for(lengths, gap=48, lead=0):
    """slots of exactly the lengths, 16-byte steps and `gap` guard bytes apart -> (dst_off, dst_cap, size)"""
    off, at = [], 64 + lead
    for n in lengths:
        off.append(at)
        at += (n + 15) // 16 * 16 + gap
    return off, list(lengths), at + 64


def check_both(eng, srcs, streams, indexes, ranges):
    """the host call and the device plan"""
    check_call(eng, srcs, streams, indexes, ranges)
    lengths = [len(want_slice(srcs[s], off, n)) for s, off, n in ranges]
    doff, dcap, size = slots_for(lengths, lead=3)
    lens, sts, _ = run_plan(eng, srcs, streams, indexes, ranges, doff, dcap, size)
    assert sts == [OK] * len(ranges) and lens == lengths


# ---- range shapes ----
SHAPE_SIZE = 200000  # six blocks of 32768 and a part


def shape_ranges():
    n = SHAPE_SIZE
    return [
        (0, 40000, 1000),           # inside one block: head edge = tail edge
        (0, 2 * BB, BB),            # exactly one block
        (0, BB, 3 * BB),            # blocks 1 to 3 exactly
        (0, 2 * BB - 1, 2),         # the last byte of block 1 and the first of block 2
        (0, 0, n),                  # the whole stream
        (0, 12345, 0),              # no bytes
        (0, n, 10),                 # off == total
        (0, n + 77, 10),            # off > total
        (0, n - 100, 5000),         # past the end: clipped
        (0, 70000, M64 - 5),        # off + len beyond 2^64
        (0, n - 1, M64),            # ... with the largest length
    ]


def check_shapes(eng, make):
    src = mix(SHAPE_SIZE)
    blob, idx = make(src, 1, oracle.dfGzip, BB)
    assert len(idx) == 8 and idx[-1][1] == SHAPE_SIZE
    ranges = shape_ranges()
    check_both(eng, [src], [blob], [idx], ranges)
    # alone: blocks 1 to 3 go straight into the slot; a range inside a block decodes it once
    check_call(eng, [src], [blob], [idx], [ranges[2]])
    assert eng.debug_range_stats()[1:] == (3, 0)
    check_call(eng, [src], [blob], [idx], [ranges[0]])
    assert eng.debug_range_stats()[1:] == (0, 1)
    check_call(eng, [src], [blob], [idx], [ranges[3]])
    assert eng.debug_range_stats()[1:] == (0, 2)
    check_call(eng, [src], [blob], [idx], [(0, BB - 1, 2 * BB + 2)])  # two edges around two whole blocks
    assert eng.debug_range_stats()[1:] == (2, 2)
    check_call(eng, [src], [blob], [idx], ranges[5:8])  # nothing to decode, nothing to upload
    assert eng.debug_range_stats() == (0, 0, 0)
    # a closing entry whose bit_off says nothing sensible: the span ends with the stream
    check_call(eng, [src], [blob], [idx[:-1] + [(M64, SHAPE_SIZE)]], [ranges[8], ranges[0]])
    assert eng.debug_range_stats()[0] <= len(blob) + 30
    assert eng.uncompress_ranges([blob], [idx], []) == ([], [])
    assert eng.uncompress_ranges([], [], []) == ([], [])


# ---- formats and levels ----
def format_streams(make):
    rnd = np.random.default_rng(77).integers(0, 256, 140000, dtype=np.uint8).tobytes()
    srcs = [mix(70000, 1), mix(70000, 2), mix(70000, 3), rnd, b"", b"zippy"]
    made = [make(srcs[0], 1, oracle.dfGzip, BB), make(srcs[1], -2, oracle.dfZlib, BB),
            make(srcs[2], 6, oracle.dfDeflate, BB), make(srcs[3], 0, oracle.dfGzip, 131072),
            make(srcs[4], 1, oracle.dfGzip, BB), make(srcs[5], 1, oracle.dfZlib, BB)]
    assert len(made[3][1]) > 3  # (stored chunks of 65535: several entries for one logical block of 131072)
    return srcs, [m[0] for m in made], [m[1] for m in made]


def check_formats(eng, make):
    srcs, streams, indexes = format_streams(make)
    rng = random.Random(11)
    ranges = []
    for k in range(5):
        for s, src in enumerate(srcs):  # (interleaved over the streams)
            n = len(src)
            ranges.append((s, rng.randrange(n + 10), rng.randrange(1, 50000)) if k else (s, 0, n + 5))
    ranges += [(3, 65534, 3), (3, 65535, 65535), (3, 131071, 2), (5, 1, 3), (4, 0, 0)]
    check_both(eng, srcs, streams, indexes, ranges)


# ---- clip alignment (the device plan) ----
CLIP_LENGTHS = (0, 1, 15, 16, 17, 31, 33, 4097)
CLIP_SIZE = 100000  # three blocks of 32768 and one of 1696: the short ranges sit in that one


def check_clip_alignment(eng, make):
    """every alignment of a clip's first source byte in the scratch (an edge block starts at a multiple of 256 there,
    so it is (off - the block's first byte) & 15) x every alignment of the slot x the lengths around 16 and one of
    more than a workgroup's 16 steps; guard bytes around every slot"""
    src = pattern(CLIP_SIZE)
    blob, idx = make(src, 1, oracle.dfDeflate, BB)
    assert [e[1] for e in idx] == [0, BB, 2 * BB, 3 * BB, CLIP_SIZE]  # (multiples of 16: off & 15 is the alignment in the block)
    ranges, doff, at, k = [], [], 64, 0
    for length in CLIP_LENGTHS:
        for s_al in range(16):
            for d_al in range(16):
                if length <= 33:
                    off = 3 * BB + 16 * (k % 90) + s_al
                else:  # inside one block, across a block start, up to the stream's end
                    off = (BB * (k % 2) + 16 * (k % 1700), 2 * BB - 16 * (1 + k % 200), CLIP_SIZE - 4097 - 15)[k % 3] + s_al
                k += 1
                assert off % 16 == s_al and off + length <= CLIP_SIZE
                ranges.append((0, off, length))
                doff.append(at + d_al)
                at += (length + 15) // 16 * 16 + 64
    lens, sts, _ = run_plan(eng, [src], [blob], [idx], ranges, doff, [r[2] for r in ranges], at + 64)
    assert sts == [OK] * len(ranges) and lens == [r[2] for r in ranges]


# ---- crafted streams ----
def _lits(s, data):
    for b in data:
        s.lit(b)
    s.eob()


def _simple_dynamic(s, final):
    lit = [8] * 254 + [9, 9, 8]  # complete: 255 codes of 8 bits and two of 9
    assert dc.kraft(lit) == 32768
    s.dynamic_block(lit, [1, 1], final)


def crafted():
    """-> [(name, raw deflate, index, plain)]: the index from bitpos in front of every block"""
    out = []
    s, idx = dc.Stream(), []
    idx.append((s.bitpos, len(s.out)))
    s.fixed_block(False)
    _lits(s, b"The quick brown fox jumps over the lazy dog. " * 3)
    idx.append((s.bitpos, len(s.out)))
    s.stored(b"", False, pad_bits=0x7f)
    idx.append((s.bitpos, len(s.out)))
    s.fixed_block(True)
    _lits(s, bytes(range(200, 256)) + b"pack my box with five dozen liquor jugs")
    idx.append((s.bitpos, len(s.out)))
    raw, plain, st = s.finish()
    assert st is None and idx[1][1] == idx[2][1]
    out.append(("empty-stored-between-fixed", raw, idx, plain))
    phases = set()
    for j in range(8):  # j nine-bit literals move the dynamic block's header through the eight bit phases
        s, idx = dc.Stream(), []
        idx.append((s.bitpos, 0))
        s.fixed_block(False)
        _lits(s, bytes([0x90 + i for i in range(j)]) + b"ab")
        idx.append((s.bitpos, len(s.out)))
        phases.add(s.bitpos % 8)
        _simple_dynamic(s, False)
        _lits(s, bytes((37 * i + j) % 256 for i in range(300)))
        idx.append((s.bitpos, len(s.out)))
        s.fixed_block(True)
        _lits(s, b"tail %d" % j)
        idx.append((s.bitpos, len(s.out)))
        raw, plain, st = s.finish()
        assert st is None
        out.append(("dynamic-at-bit-%d" % (idx[1][0] % 8), raw, idx, plain))
    assert phases == set(range(8))
    return out


def check_crafted(eng):
    cases = crafted()
    srcs, streams, indexes = [x[3] for x in cases], [x[1] for x in cases], [x[2] for x in cases]
    ranges = []
    for s, (_, _, idx, plain) in enumerate(cases):
        ranges.append((s, 0, len(plain) + 1))
        for bit, at in idx[1:-1]:  # across every block boundary, and up to / from it
            ranges += [(s, at - 1, 2), (s, max(0, at - 5), 5), (s, at, 4), (s, at - 1, 1), (s, at, 1)]
    check_both(eng, srcs, streams, indexes, ranges)


# ---- failures ----
def seven_blocks(make):
    src = mix(7 * BB - 1000, 5)
    blob, idx = make(src, 1, oracle.dfGzip, BB)
    assert len(idx) == 8
    return src, blob, idx


def block_ranges(nblocks, total):
    """per block: a range inside it, the block itself, and one that runs from the block before into the block behind"""
    out = []
    for k in range(nblocks):
        out += [(0, k * BB + 100, 300), (0, k * BB, BB), (0, max(0, k * BB - 10), BB + 20)]
    return out


def touches(rng, lo, hi, total):
    """the range has a byte in [lo, hi)"""
    a, b = rng[1], min(total, rng[1] + rng[2])
    return a < b and a < hi and lo < b


def check_damaged_block(eng, make):
    """two bytes wrong inside block 3 of 7: the ranges that touch it fail with the status the indexed decode of the
    whole stream gives for that block (read as raw deflate: no container check in front of it), or with
    ZH_ERR_INVALID_BUFFER per the mapping; every other range returns the right bytes"""
    from zippy_amd.common import ZippyError
    src, blob, idx = seven_blocks(make)
    at = (idx[3][0] // 8 + idx[4][0] // 8) // 2
    damaged = bytearray(blob)
    damaged[at] ^= 0xff
    damaged[at + 1] ^= 0xff
    damaged = bytes(damaged)
    try:
        eng.uncompress_indexed(damaged, idx, oracle.dfDeflate)  # (no container: the block's status comes through)
        whole = None
    except ZippyError as e:
        whole = e.status
    ranges = block_ranges(7, len(src))
    bad = {r for r, x in enumerate(ranges) if touches(x, 3 * BB, 4 * BB, len(src))}
    assert 3 <= len(bad) < len(ranges)
    outs, sts = check_call(eng, [src], [damaged], [idx], ranges, bad)
    for r in bad:
        assert outs[r] is None and sts[r] != OK
        if sts[r] != INVALID_BUFFER:
            assert sts[r] == whole, (r, sts[r], whole)
    return src, damaged, idx


def check_moved_entry(eng, make):
    """entry 3's out_off one too large: block 2 promises a byte more than it makes, block 3 one less"""
    src, blob, idx = seven_blocks(make)
    moved = list(idx)
    moved[3] = (idx[3][0], idx[3][1] + 1)
    ranges = block_ranges(7, len(src))
    bad = {r for r, x in enumerate(ranges) if touches(x, 2 * BB, 4 * BB, len(src))}
    outs, sts = check_call(eng, [src], [blob], [moved], ranges, bad)
    assert all(sts[r] == INVALID_BUFFER and outs[r] is None for r in bad)


def check_bad_index_of_one_stream(eng, make):
    srcs = [mix(70000, 1), mix(70000, 2), mix(70000, 3)]
    made = [make(x, 1, oracle.dfGzip, BB) for x in srcs]
    streams = [m[0] for m in made]
    ranges = [(s, off, n) for off, n in ((0, 70000), (100, 10), (40000, 30000), (70000, 1), (5, 0)) for s in range(3)]
    good = made[1][1]
    for bad_idx in ([good[0], good[2], good[1], good[3]],                 # entries out of order
                    good[:1],                                             # a single entry
                    [],                                                   # none
                    [(good[0][0], 1)] + good[1:],                         # entry 0 not at output byte 0
                    good[:2] + [(8 * len(streams[1]), good[2][1])] + good[3:],  # a block that starts behind the stream
                    good[:2] + [(good[2][0], 10 ** 9), (good[3][0], 10 ** 9 + 10)]):  # 1e9 bytes out of 20 KB
        indexes = [made[0][1], bad_idx, made[2][1]]
        bad = {r for r, x in enumerate(ranges) if x[0] == 1}
        outs, sts = check_call(eng, srcs, streams, indexes, ranges, bad)
        assert all(sts[r] == INVALID_BUFFER and outs[r] is None for r in bad), (bad_idx[:4], sts)


def check_call_errors(eng, make):
    from zippy_amd.common import ZippyError
    src = mix(70000, 1)
    blob, idx = make(src, 1, oracle.dfGzip, BB)
    for ranges in ([(1, 0, 5)], [(0, 0, 5), (M64, 0, 5)]):
        try:
            eng.uncompress_ranges([blob], [idx], ranges)
            raise AssertionError("no error")
        except ZippyError as e:
            assert e.status == ARGUMENT
        try:
            eng.plan_uncompress_ranges([0], [len(blob)], [idx], ranges, [0] * len(ranges), [5] * len(ranges))
            raise AssertionError("no error")
        except ZippyError as e:
            assert e.status == ARGUMENT
    # NULL arrays, straight at the C ABI
    lib, h = eng.lib, eng._h
    one = (c.c_uint64 * 1)(0)
    first = (c.c_size_t * 2)(0, len(idx))
    flat = (c.c_uint64 * (2 * len(idx)))(*[v for e in idx for v in e])
    p = c.c_void_p()
    ln = (c.c_uint64 * 1)(len(blob))
    assert lib.zh_plan_uncompress_ranges(h, 1, one, ln, flat, first, 1, None, one, one, one, one, c.byref(p)) == ARGUMENT
    assert lib.zh_plan_uncompress_ranges(h, 1, one, ln, flat, first, 1, one, one, one, None, one, c.byref(p)) == ARGUMENT
    assert lib.zh_plan_uncompress_ranges(h, 1, one, ln, None, first, 1, one, one, one, one, one, c.byref(p)) == ARGUMENT
    assert lib.zh_plan_uncompress_ranges(h, 1, one, ln, flat, first, 1, one, one, one, one, one, None) == ARGUMENT
    srcs = (c.c_void_p * 1)(c.cast(c.c_char_p(blob), c.c_void_p))
    lens = (c.c_size_t * 1)(len(blob))
    d, dl, st = (c.c_void_p * 1)(), (c.c_size_t * 1)(), (c.c_int32 * 1)()
    assert lib.zh_uncompress_ranges(h, srcs, lens, 1, flat, first, 1, one, one, None, d, dl, st) == ARGUMENT
    assert lib.zh_uncompress_ranges(h, srcs, lens, 1, flat, first, 1, one, one, one, None, dl, st) == ARGUMENT
    assert lib.zh_uncompress_ranges(h, None, lens, 1, flat, first, 1, one, one, one, d, dl, st) == ARGUMENT
    assert lib.zh_debug_range_stats(None, None, None, None) == ARGUMENT


def check_plan_refuses_other_calls(eng, make):
    src = mix(70000, 1)
    blob, idx = make(src, 1, oracle.dfGzip, BB)
    plan = eng.plan_uncompress_ranges([0], [len(blob)], [idx], [(0, 0, 10)], [0], [10])
    try:
        lib, h = eng.lib, plan._h
        x = c.c_void_p(256)
        assert lib.zh_plan_pack(h, x, x, 1 << 20, x) == ARGUMENT
        assert lib.zh_plan_unpack(h, x, x, x) == ARGUMENT
        assert lib.zh_plan_set_src_lens_device(h, x) == ARGUMENT
        assert lib.zh_plan_request_crc32(h, 1) == ARGUMENT
        i, n = c.POINTER(c.c_uint64)(), c.c_size_t()
        assert lib.zh_plan_block_index(h, 0, c.byref(i), c.byref(n)) == ARGUMENT
    finally:
        plan.close()


def check_small_slot(eng, make):
    """a slot smaller than its clipped range: that range's status and the size it needs; its neighbours are whole and
    nothing of it is written"""
    src = mix(SHAPE_SIZE)
    blob, idx = make(src, 1, oracle.dfGzip, BB)
    ranges = [(0, 1000, 3000), (0, BB - 5, BB + 10), (0, 5 * BB, 10 ** 9), (0, 70000, 64)]
    lengths = [len(want_slice(src, off, n)) for _, off, n in ranges]
    doff, dcap, size = slots_for(lengths)
    dcap[1] -= 1
    dcap[2] = 17
    lens, sts, stats = run_plan(eng, [src], [blob], [idx], ranges, doff, dcap, size)
    assert sts == [OK, DST_TOO_SMALL, DST_TOO_SMALL, OK]
    assert lens == lengths
    assert stats == (0, 0, 2)  # (the two refused ranges: none of their blocks)


# ---- upload accounting ----
def spans_of(indexes, lens, ranges):
    """per range the compressed bytes [bit_off[k0] / 8, ceil(bit_off[k1 + 1] / 8)) of its stream, from the index alone
    -> (S: the spans' lengths summed, U: the length of their union stream by stream)"""
    per = {}
    total = 0
    for s, off, n in ranges:
        idx = indexes[s]
        end = min(idx[-1][1], off + n)
        if off >= end:
            continue
        ks = [k for k in range(len(idx) - 1) if idx[k][1] < end and idx[k + 1][1] > off]
        lo, hi = idx[ks[0]][0] // 8, min(lens[s], (idx[ks[-1] + 1][0] + 7) // 8)
        total += hi - lo
        per.setdefault(s, []).append((lo, hi))
    union = 0
    for spans in per.values():
        spans.sort()
        at = 0
        for lo, hi in spans:
            union += max(0, hi - max(lo, at))
            at = max(at, hi)
    return total, union


def check_upload_accounting(eng, make):
    """The library sends every merged span from the next multiple of 16 of one buffer: at most 15 bytes of padding a
    span, and never more spans than ranges."""
    srcs, streams, indexes = format_streams(make)
    lens = [len(x) for x in streams]
    for ranges in accounting_sets(srcs):
        check_call(eng, srcs, streams, indexes, ranges)
        up = eng.debug_range_stats()[0]
        S, U = spans_of(indexes, lens, ranges)
        assert U <= up <= S + 64 * len(ranges), (ranges, U, up, S)
        assert up <= U + 15 * len(ranges)
    src = mix(1 << 18, 6)
    blob, idx = make(src, 1, oracle.dfGzip, BB)
    ranges = [(0, 100000, 4096)]
    S, U = spans_of([idx], [len(blob)], ranges)
    assert S + 64 < len(blob) // 4  # (from the index: a 4 KiB range needs one block of eight, or two)
    check_call(eng, [src], [blob], [idx], ranges)
    assert U <= eng.debug_range_stats()[0] <= S + 64 < len(blob) // 4


# ---- the cases as files, for tests/ranges_sanitize_main.cpp ----
def accounting_sets(srcs):
    """the five sets of ranges of check_upload_accounting over format_streams()"""
    rng = random.Random(5)
    return [[(0, 100, 10)],
            [(0, 100, 10), (0, 200, 10)],                      # the same block twice: sent once
            [(0, 0, BB), (0, BB, BB)],                         # neighbours: they touch
            [(s, rng.randrange(len(srcs[s])), rng.randrange(1, 40000)) for s in (3, 0, 2, 1, 0, 3, 2, 1, 5)],
            [(0, 0, 70000), (1, 69999, 1), (4, 0, 1)]]


def dump(path):
    """shape_ranges(), the damaged block, the unsound indexes of one stream among three and the five sets of the
    upload's accounting, streams and indexes from the oracle.  cases.txt: "NAME STREAMS U" a line (U: the union of the
    spans the call must send, -1: not held against the counter); NAME_<s>.bin / .idx ("BIT_OFF OUT_OFF" a line) / .src
    per stream; NAME.ranges: "STREAM OFF LEN STATUS" a line -- 0: the slice of .src; -1: a status of the decoder's;
    else that status.  -> the number of (cases, ranges)"""
    import os
    os.makedirs(path)

    def put(name, data):
        with open(os.path.join(path, name), "wb") as f:
            f.write(data)

    cases = []  # (name, srcs, streams, indexes, [(stream, off, len, status)], U)

    def add(name, srcs, streams, indexes, ranges, bad=(), bad_status=INVALID_BUFFER, account=False):
        U = spans_of(indexes, [len(x) for x in streams], ranges)[1] if account else -1
        cases.append((name, srcs, streams, indexes,
                      [x + (bad_status if r in bad else OK,) for r, x in enumerate(ranges)], U))

    src = mix(SHAPE_SIZE)
    blob, idx = make_oracle(src, 1, oracle.dfGzip, BB)
    add("shapes", [src], [blob], [idx], shape_ranges(), account=True)

    src, blob, idx = seven_blocks(make_oracle)
    at = (idx[3][0] // 8 + idx[4][0] // 8) // 2
    damaged = bytearray(blob)
    damaged[at] ^= 0xff
    damaged[at + 1] ^= 0xff
    try:
        oracle.uncompress(bytes(damaged), oracle.dfGzip)
        raise AssertionError("the oracle decodes the damaged stream")
    except oracle.ZippyError:
        pass
    ranges = block_ranges(7, len(src))
    bad = {r for r, x in enumerate(ranges) if touches(x, 3 * BB, 4 * BB, len(src))}
    assert 3 <= len(bad) < len(ranges)
    add("damaged", [src], [bytes(damaged)], [idx], ranges, bad, -1)

    srcs = [mix(70000, 1), mix(70000, 2), mix(70000, 3)]
    made = [make_oracle(x, 1, oracle.dfGzip, BB) for x in srcs]
    streams = [m[0] for m in made]
    ranges = [(s, off, n) for off, n in ((0, 70000), (100, 10), (40000, 30000), (70000, 1), (5, 0)) for s in range(3)]
    good = made[1][1]
    for k, bad_idx in enumerate(([good[0], good[2], good[1], good[3]], good[:1], [], [(good[0][0], 1)] + good[1:],
                                 good[:2] + [(8 * len(streams[1]), good[2][1])] + good[3:],
                                 good[:2] + [(good[2][0], 10 ** 9), (good[3][0], 10 ** 9 + 10)])):
        add("badindex%d" % k, srcs, streams, [made[0][1], bad_idx, made[2][1]], ranges,
            {r for r, x in enumerate(ranges) if x[0] == 1})

    srcs, streams, indexes = format_streams(make_oracle)
    for k, ranges in enumerate(accounting_sets(srcs)):
        add("accounting%d" % k, srcs, streams, indexes, ranges, account=True)

    for name, srcs, streams, indexes, ranges, U in cases:
        for s in range(len(streams)):
            put("%s_%d.bin" % (name, s), streams[s])
            put("%s_%d.src" % (name, s), srcs[s])
            put("%s_%d.idx" % (name, s), "".join("%d %d\n" % e for e in indexes[s]).encode())
        put(name + ".ranges", "".join("%d %d %d %d\n" % x for x in ranges).encode())
    put("cases.txt", "".join("%s %d %d\n" % (c[0], len(c[2]), c[5]) for c in cases).encode())
    return len(cases), sum(len(c[4]) for c in cases)


# ---- scratch groups ----
def straddling_ranges(n, total):
    """n ranges that each cut into two blocks of 32768"""
    nb = total // BB
    return [(0, BB * (1 + k % (nb - 1)) - 100 - k, 200 + 3 * k) for k in range(n)]
