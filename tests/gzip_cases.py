"""Shared by tests/test_emu_gzip.py and tests/test_gpu_gzip.py: gzip images of any shape made member by member, and the
checks of zh_gzip_read_batch (Engine.gzip_read_batch) against tests/gzip_model.py -- statuses, data and every field of
every member record.  Where zlib rejects a stream, the status to equal is the one Engine.uncompress_batch gives the same
bytes as raw deflate.  Every check takes `budget`: None runs the call as it is, a number sets ZH_GZIP_SPEC_BYTES, the
speculative sizing pass's budget of input bytes (0: every member is sized by frontier rounds) -- same results.

The geometry behind the sizes: the scan reads 16-byte chunks, a wave 1024 bytes, a workgroup 16384 (zh_scan.h); the NUL
search of the header kernel takes 64 bytes a step; batches of more than ZH_INFLATE_WIDE candidates (768; the emulator's
engine: 3) size with the narrow kernels."""
import contextlib
import glob
import os
import random
import struct
import zlib

import deflate_craft as dc
import gzip_model as gm

HERE = os.path.dirname(os.path.abspath(__file__))
SUPER = 64 * 1024  # the widest kernel's superchunk: what a workgroup may consume between two looks at the budget


def pattern(n, seed=1):
    """text-like bytes with long and short repeats, some noise in between"""
    rng = random.Random(seed * 7919 + n)
    out = bytearray()
    words = [bytes(rng.randrange(97, 123) for _ in range(rng.randrange(2, 9))) for _ in range(40)]
    while len(out) < n:
        k = rng.randrange(10)
        if k == 0:
            out += bytes(rng.randrange(256) for _ in range(rng.randrange(1, 60)))
        elif k == 1:
            out += bytes([rng.randrange(256)]) * rng.randrange(1, 300)
        else:
            out += rng.choice(words) + b" "
    return bytes(out[:n])


def deflate(plain, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(plain) + c.flush()


def member(plain=b"", level=6, raw=None, extra=None, name=None, comment=None, hcrc=False, mtime=0, xfl=0, os_=255,
           ftext=False, crc=None, isize=None, hcrc_xor=0):
    """one gzip member; raw: its deflate bytes (then `plain` is what they make); crc / isize / hcrc_xor plant faults"""
    flg = (gm.FTEXT if ftext else 0) | (gm.FHCRC if hcrc else 0) | (gm.FEXTRA if extra is not None else 0) | \
          (gm.FNAME if name is not None else 0) | (gm.FCOMMENT if comment is not None else 0)
    head = bytes([0x1f, 0x8b, 8, flg]) + struct.pack("<IBB", mtime, xfl, os_)
    if extra is not None:
        head += struct.pack("<H", len(extra)) + extra
    if name is not None:
        head += name + b"\0"
    if comment is not None:
        head += comment + b"\0"
    if hcrc:
        head += struct.pack("<H", (zlib.crc32(head) & 0xffff) ^ hcrc_xor)
    body = deflate(plain, level) if raw is None else raw
    return head + body + struct.pack("<II", zlib.crc32(plain) if crc is None else crc,
                                     len(plain) & 0xffffffff if isize is None else isize)


def members(k, seed=0, size=300):
    """k members of mixed levels, sizes and header fields"""
    out = []
    for i in range(k):
        plain = pattern((size * ((i * 7 + seed) % 5 + 1)) // 3 if (i + seed) % 9 else 0, seed * 100 + i)
        out.append(member(plain, level=(0, 1, 6, 9)[(i + seed) % 4], name=b"m%d" % i if i % 3 == 0 else None,
                          extra=b"\x01\x02\x03"[:i % 4] if i % 5 == 1 else None, hcrc=i % 7 == 2, mtime=i * 1000003 + seed))
    return out


@contextlib.contextmanager
def spec_budget(budget):
    old = os.environ.get("ZH_GZIP_SPEC_BYTES")
    if budget is not None:
        os.environ["ZH_GZIP_SPEC_BYTES"] = str(budget)
    try:
        yield
    finally:
        if budget is not None:
            if old is None:
                del os.environ["ZH_GZIP_SPEC_BYTES"]
            else:
                os.environ["ZH_GZIP_SPEC_BYTES"] = old


def decoder_status(eng):
    cache = {}

    def status(src):
        if src not in cache:
            cache[src] = eng.uncompress_batch([src], 3)[1][0]
        return cache[src]
    return status


def check(eng, images, budget=None, want=None, sound=None, list_alone=True):
    """one call over `images`: everything equals the model's; want: the statuses expected (a check of the case itself);
    sound: True when every image must be sound; list_alone: the call once more for the member list without data"""
    dec = decoder_status(eng)
    model = [gm.read(im, dec) for im in images]
    if want is not None:
        assert [m[0] for m in model] == list(want), ([m[0] for m in model], want)
    if sound:
        assert all(m[0] == gm.OK for m in model), [m[0] for m in model]
    with spec_budget(budget):
        outs, sts, mems = eng.gzip_read_batch(images)
        stats = eng.debug_gzip_stats()
        outs2, sts2, mems2 = eng.gzip_read_batch(images, want_data=False) if list_alone else ([None] * len(images), sts, mems)
    assert sts == [m[0] for m in model], (sts, [m[0] for m in model])
    assert sts2 == sts and mems2 == mems and outs2 == [None] * len(images)
    for i, (st, data, recs) in enumerate(model):
        if st != gm.OK:
            assert outs[i] is None and mems[i] is None, i
            continue
        assert outs[i] == data, i
        assert mems[i] == recs, (i, [(a, b) for a, b in zip(mems[i], recs) if a != b][:3], len(mems[i]), len(recs))
    return stats


# ---------------------------------------------------------------------------
# chain length
# ---------------------------------------------------------------------------
def check_chain_lengths(eng, budget=None):
    images = [b"".join(members(k, seed=k)) for k in (0, 1, 2, 3, 64, 65)]
    check(eng, images, budget, sound=True)
    for im in images:
        check(eng, [im], budget, sound=True)


def check_batch_33(eng, budget=None):
    images = []
    for i in range(33):
        k = (0, 1, 5, 2, 0, 17, 3)[i % 7]
        images.append(b"".join(members(k, seed=i, size=200 + 150 * (i % 6))))
    assert images.count(b"") >= 2
    check(eng, images, budget, sound=True)


def check_1600_members(eng, budget=None):
    image = b"".join(member(pattern(40 + i % 23, i), level=(1, 6)[i & 1]) for i in range(1600))
    stats = check(eng, [image], budget, sound=True)
    assert stats[0] >= 1600  # (more candidates than the wide kernels take: the narrow width)


def fixtures(limit=None):
    paths = sorted(glob.glob(os.path.join(HERE, "golden", "**", "*.gz"), recursive=True))
    blobs = [open(p, "rb").read() for p in paths]
    return [b for b in blobs if limit is None or len(b) <= limit]


def check_fixtures(eng, budget=None, list_alone=True):
    blobs = fixtures()
    assert len(blobs) == 24  # (every .gz under tests/golden, the tarball of 3.9 MB among them)
    check(eng, [b"".join(blobs)] + blobs, budget, list_alone=list_alone)


# ---------------------------------------------------------------------------
# where a stream ends
# ---------------------------------------------------------------------------
DYN_LIT = [0] * 97 + [1, 2] + [0] * 157 + [2]  # 'a': 1 bit, 'b': 2 bits, end of block: 2 bits
DYN_DIST = [1, 1]


def crafted_streams():
    """raw deflate streams whose final block ends at each of the 8 bit residues of its last byte, for a fixed, a dynamic
    and a stored final block (a stored block ends on a byte: there its HEADER stands at each residue)"""
    out = []
    for kind in ("fixed", "dynamic", "stored"):
        seen = set()
        for k in range(40):
            s = dc.Stream()
            if kind == "fixed":
                s.fixed_block(True)
                for j in range(k):
                    s.lit(0x41 + j % 3 if j % 2 else 0x91)  # 8- and 9-bit codes
                s.eob()
                res = s.bitpos % 8
            elif kind == "dynamic":
                s.dynamic_block(DYN_LIT, DYN_DIST, True)
                for j in range(k + 1):
                    s.lit(97)
                s.eob()
                res = s.bitpos % 8
            else:
                s.fixed_block(False)
                for j in range(k):
                    s.lit(0x41 if j % 2 else 0x91)
                s.eob()
                res = s.bitpos % 8
                s.stored(bytes(range(k)), True, pad_bits=0x55)
            if res in seen:
                continue
            seen.add(res)
            s.final_pad = 0x7f  # (what the bits behind the stream hold is nobody's business)
            raw, plain, st = s.finish()
            assert st is None and zlib.decompress(raw, -15) == plain
            out.append((kind, res, raw, plain))
        assert seen == set(range(8)), (kind, seen)
    return out


def check_stream_ends(eng, budget=None):
    crafted = crafted_streams()
    tail = member(pattern(100, 5))
    images = [member(plain, raw=raw) + tail for _, _, raw, plain in crafted]
    images.append(b"".join(member(plain, raw=raw) for _, _, raw, plain in crafted))
    empty = member(b"")
    assert len(empty) == 20
    images += [empty, empty * 3, tail + empty + tail, empty + tail]
    big = random.Random(11).randbytes(65535)
    s = dc.Stream()
    s.stored(big, True)
    raw, plain, _ = s.finish()
    images.append(member(plain, raw=raw) + tail)
    images.append(tail + member(plain, raw=raw))
    check(eng, images, budget, sound=True)


# ---------------------------------------------------------------------------
# headers
# ---------------------------------------------------------------------------
def check_header_fields(eng, budget=None):
    plain = pattern(500, 2)
    images = []
    for f in range(16):  # every combination of FEXTRA / FNAME / FCOMMENT / FHCRC
        m = member(plain, extra=b"ab\x03\x00xyz" if f & 1 else None, name=b"file.txt" if f & 2 else None,
                   comment=b"a comment" if f & 4 else None, hcrc=bool(f & 8))
        images.append(m + member(b"next") + m)
    for xlen in (0, 1, 65535):
        images.append(member(plain, extra=bytes(xlen % 251 for _ in range(xlen))) + member(b"behind", hcrc=True, extra=b"\0" * xlen))
    for nlen in (0, 1, 63, 64, 65, 4097):  # either side of the NUL search's step
        nm = bytes(0x61 + i % 26 for i in range(nlen))
        images.append(member(plain, name=nm) + member(plain, comment=nm) + member(plain, name=nm, comment=nm[::-1], hcrc=True))
    images.append(member(plain, ftext=True, mtime=0xfedcba98, xfl=4, os_=3) + member(plain, ftext=True, hcrc=True, xfl=2, os_=0, mtime=1))
    check(eng, images, budget, sound=True)
    good = member(plain, name=b"n", hcrc=True)
    bad = [member(plain, name=b"n", hcrc=True, hcrc_xor=x) for x in (0x0001, 0x0100, 0x8000)]
    images = [good] + bad + [good + b + good for b in bad]
    check(eng, images, budget, want=[gm.OK] + [gm.CHECKSUM] * 6)


def check_bgzf_as_gzip(eng, budget=None):
    srcs = [pattern(3 * 4096 + 77, 9), b"", pattern(100, 3)]
    files, sts = eng.bgzf_compress_batch(srcs, 6, 4096)
    assert sts == [0, 0, 0]
    check(eng, files + [files[0] + files[2]], budget, sound=True)
    outs, _, mems = eng.gzip_read_batch(files)
    assert outs == srcs and [len(m) for m in mems] == [5, 1, 2]
    assert all(m["flg"] == 4 and m["extra_len"] == 6 for m in mems[0])


# ---------------------------------------------------------------------------
# false candidates
# ---------------------------------------------------------------------------
def stored_member(payload):
    """a member whose deflate stream is stored blocks over `payload`: the payload stands in the image byte for byte"""
    s = dc.Stream()
    for o in range(0, max(len(payload), 1), 65535):
        s.stored(payload[o:o + 65535], o + 65535 >= len(payload))
    raw, plain, _ = s.finish()
    return member(plain, raw=raw)


def check_false_candidates(eng, budget=None):
    inner = member(pattern(700, 4), name=b"inner.txt")
    real = member(pattern(300, 6))
    images = [
        stored_member(inner) + real,                  # a complete valid .gz inside a stored block
        stored_member(inner + inner) + stored_member(b"x" + inner),
        stored_member(b"\x1f\x8b\x08\x08" + b"no NUL before the image ends " * 3) + stored_member(b"\x1f\x8b\x08\x18abc"),
        stored_member(b"\x1f\x8b\x08\x00" + random.Random(5).randbytes(400)) + real,
        stored_member(random.Random(6).randbytes(100) + b"\x1f\x8b\x08\x00" + random.Random(7).randbytes(40)),
    ]
    check(eng, images, budget, sound=True)
    # A candidate exactly one byte before and one byte behind the place where a real member ends.  The byte a member
    # ends at cannot belong to two signatures, so no such image is sound: one byte early the ISIZE's top byte is the
    # candidate's 1f (a forged ISIZE), one byte late a stray byte stands between the members.  The verdict is the
    # model's: that of the real chain, whatever the candidate next to it decodes to.
    a, q = member(pattern(200, 8)), member(b"q" * 50)
    images = [a[:-1] + q, a[:-1] + q + real, a + b"\0" + q, a + b"\x1f" + q + real, real + a[:-1] + q]
    stats = check(eng, images, budget, want=[gm.SIZE, gm.SIZE, gm.GZIP_ID, gm.GZIP_ID, gm.SIZE])
    assert stats[0] >= 7


def straddling_images():
    """-> (images, places): 32 images whose second member starts at every residue of 16 (the first member's name pads
    it to the byte), and three pairs of images with a signature across their boundary: image 0 ends with the first k
    bytes of a signature, image 1 starts with the rest, and neither holds a member there.  places[i]: where image i's
    second member starts."""
    images, places = [], []
    for r in range(32):
        base = member(pattern(50 + r, r), name=b"")
        first = member(pattern(50 + r, r), name=b"n" * ((r - len(base)) % 16))
        assert len(first) % 16 == r % 16
        im = first + member(pattern(60, r + 20)) + member(b"")
        # (zeros behind the last member are a clean end: they keep the next image of a batch at a multiple of 16 of
        # the upload, from the 17th image on at 8 more)
        images.append(im + b"\0" * ((-len(im)) % 16 + (8 if r >= 16 else 0)))
        places.append(len(first))
    a, b = member(pattern(90, 1)), member(pattern(80, 2))
    for k in (1, 2, 3):
        images.append(a + b[:k])
        images.append(b[k:])
    return images, places


def upload_residues(images, places):
    """the residues of 16 at which the second members' signatures stand in ONE upload of the images: image t lies at the
    sum of the lengths before it, each rounded up to 8 (zh_scan.h: scan_upload)"""
    out, up = set(), 0
    for im, at in zip(images, places):
        out.add((up + at) % 16)
        up += (len(im) + 7) & ~7
    return out


def check_straddling(eng, budget=None):
    images, places = straddling_images()
    # one image a call: the image lies at byte 0 of the upload, the second member's signature at its own residue
    assert {at % 16 for at in places[:16]} == set(range(16))
    for im in images[:16]:
        check(eng, [im], budget, sound=True)
    # all in one call: residue 15 is one byte in one chunk and three in the next, 13 and 14 likewise two and one
    assert upload_residues(images, places) == set(range(16))
    check(eng, images, budget)
    check(eng, images[:32], budget, sound=True)


# ---------------------------------------------------------------------------
# ends
# ---------------------------------------------------------------------------
def check_ends(eng, budget=None):
    ms = [member(pattern(400 + 50 * i, i), level=(1, 6, 9)[i % 3]) for i in range(5)]
    whole = b"".join(ms)
    images, want = [], []
    for z in (1, 7, 8, 511, 4097):
        images.append(whole + b"\0" * z)
        want.append(gm.OK)
    images.append(whole + b"\x01")
    want.append(gm.INVALID_BUFFER)
    images.append(whole + b"\x1f\x8b\x07" + b"\0" * 15)
    want.append(gm.UNSUPPORTED_METHOD)
    images.append(whole + b"\0" * 20 + b"\x01")
    want.append(gm.GZIP_ID)
    images.append(b"\0" * 18)
    want.append(gm.GZIP_ID)
    images.append(b"\0" * 5)
    want.append(gm.INVALID_BUFFER)
    for where in (0, 2, 4):  # a wrong CRC, a wrong ISIZE in the first, a middle and the last member
        for fault in ("crc", "isize"):
            bad = list(ms)
            bad[where] = member(pattern(400 + 50 * where, where), level=(1, 6, 9)[where % 3], **{fault: 12345})
            images.append(b"".join(bad))
            want.append(gm.CHECKSUM if fault == "crc" else gm.SIZE)
    check(eng, images, budget, want=want)
    # the image cut at every byte of the last member's trailer and of its last 4 deflate bytes; a damaged deflate byte
    images = [whole[:len(whole) - k] for k in range(1, 13)]
    damaged = bytearray(whole)
    at = len(ms[0]) + len(ms[1]) + 10 + 20
    damaged[at] ^= 0x55
    images.append(bytes(damaged))
    images.append(whole)  # (the neighbours of the failing images stay sound)
    check(eng, images, budget)
    with spec_budget(budget):
        _, sts, _ = eng.gzip_read_batch(images)
    assert sts[-1] == 0 and all(st != 0 for st in sts[:13]), sts


# ---------------------------------------------------------------------------
# the budget
# ---------------------------------------------------------------------------
ADV_HEADERS = 2000
ADV_BUDGET = 1 << 20


def adversarial_image():
    """Just under 256 KiB: a member whose stored blocks hold 2000 ten-byte headers, each followed by a stored block that
    reaches to ONE chain of stored blocks of 8000 bytes, which runs on to the end of the member's payload -- every header
    is a candidate whose stream reads on for the rest of the image, 2000 x ~ 235 KB in all --, and behind it a real
    member of 200 small stored blocks, the last candidate in file order: by the time its workgroup has read a few of
    its headers the budget is spent, and a frontier round has to size it.
    The container's own block headers (5 bytes every 65535 of payload) stand in the image between the payload's bytes:
    the chain is laid out in image positions and steps over them."""
    n_payload = 250000
    payload = bytearray(b"." * n_payload)

    def img(o):  # where payload byte o stands in the image
        return 10 + 5 * (o // 65535 + 1) + o

    def at(p):  # ... and back; None inside one of the container's block headers
        k, w = divmod(p - 10, 65540)
        return None if w < 5 else k * 65535 + w - 5

    def put(p, final, length):  # a stored block's header at image position p
        o = at(p)
        assert o is not None and at(p + 4) == o + 4
        payload[o:o + 5] = struct.pack("<BHH", 1 if final else 0, length, length ^ 0xffff)

    end = img(n_payload - 1) + 1
    chain = img(15 * ADV_HEADERS)
    for j in range(ADV_HEADERS):
        payload[15 * j:15 * j + 10] = b"\x1f\x8b\x08\x00" + b"\0" * 6
        p = img(15 * j + 10)
        put(p, False, chain - (p + 5))
    q = chain
    while q + 5 + 8000 + 5 + 5 <= end:
        nxt = q + 5 + 8000
        while at(nxt) is None or at(nxt + 4) is None:
            nxt += 1
        put(q, False, nxt - (q + 5))
        q = nxt
    put(q, True, end - (q + 5))
    s = dc.Stream()
    for k in range(200):
        s.stored(bytes([0x30 + k % 10]) * 50, k == 199)
    raw, plain, _ = s.finish()
    return stored_member(bytes(payload)) + member(plain, raw=raw)


def candidate_bytes(image):
    """the input bytes every candidate's stream takes when nothing stops it: (candidates, their sum)"""
    n = total = 0
    at = image.find(b"\x1f\x8b\x08")
    while at >= 0:
        st, rec = gm.header_at(image, at)
        if st == gm.OK:
            src = image[rec["cdata_off"]:max(rec["cdata_off"], len(image) - 8)]
            d = zlib.decompressobj(-15)
            try:
                d.decompress(src)
            except zlib.error:
                pass
            n += 1
            total += len(src) - len(d.unused_data)
        at = image.find(b"\x1f\x8b\x08", at + 1)
    return n, total


def resident_workgroups(candidates, compute_units):
    """The most workgroups of the sizing pass that are on the device at a time, from its launch (zh_inflate_split.hip:
    zh_launch_inflate_spec): up to 768 candidates take the 1024-thread form -- 94 KB of LDS, one a CU --, more take the
    256- and the 128-thread forms, one launch after the other: 4 waves each at 5 waves a SIMD, 5 a CU, and 2 waves each
    at 4 waves a SIMD, 8 a CU (their 31 KB / 20 KB of LDS fit as often into a CU's 160 KiB)."""
    return min(candidates, compute_units * (1 if candidates <= 768 else 8))


def check_adversarial_model():
    image = adversarial_image()
    assert 250 * 1024 <= len(image) <= 256 * 1024, len(image)
    st, data, recs = gm.read(image, lambda src: 13)
    assert st == gm.OK and len(recs) == 2 and data.count(b"\x1f\x8b\x08\x00") == ADV_HEADERS
    n, total = candidate_bytes(image)
    assert n == ADV_HEADERS + 2
    # what nothing stops is several times what the budget lets through on the largest device the tests know (256 CUs)
    assert total > 3 * (ADV_BUDGET + resident_workgroups(n, 256) * SUPER), total
    return n, total


def check_adversarial(eng, in_flight, unbudgeted_run):
    """in_flight(candidates): the workgroups of the pass that run at a time (the emulator: one); unbudgeted_run: size
    everything once more without a budget (the emulator takes minutes over it: there the model's figure stands in)"""
    image = adversarial_image()
    n, free_bytes = candidate_bytes(image)
    candidates, spec_bytes, rounds = check(eng, [image], ADV_BUDGET, sound=True)
    assert candidates == n
    # A workgroup pays for what it consumed and looks at the sum where it reads a block header or stages a superchunk:
    # at most a superchunk (64 KiB; no block of this image is longer) since its last look.  The sum reaches the budget
    # once; from then on every workgroup that is running pays once more and stops, and one that starts pays nothing.
    slack = in_flight(candidates) * SUPER
    print("adversarial: %d candidates, %d speculative bytes (budget %d, slack %d, unbudgeted %d), %d frontier rounds" %
          (candidates, spec_bytes, ADV_BUDGET, slack, free_bytes, rounds))
    assert spec_bytes <= ADV_BUDGET + slack
    assert spec_bytes >= ADV_BUDGET  # (it was the budget that stopped the pass)
    assert rounds > 0
    assert spec_bytes * 3 < free_bytes
    if unbudgeted_run:
        _, all_bytes, no_rounds = check(eng, [image], 1 << 40, sound=True)
        print("adversarial, no budget: %d speculative bytes" % all_bytes)
        assert no_rounds == 0 and abs(all_bytes - free_bytes) <= 8 * candidates and spec_bytes * 3 < all_bytes


NUL_STRIDE = 4096  # bytes of a NUL search between two payments (zh_gzip.hip)


def nameless_image(copies):
    """a member whose stored block holds 4 x copies bytes without a zero byte, 1f 8b 08 08 every four of them: `copies`
    candidates with FNAME set, each one's "name" running to the first zero behind the payload, and a real member with
    a name behind it"""
    return stored_member(b"\x1f\x8b\x08\x08" * copies) + member(pattern(300, 3), name=b"real")


def check_nul_search_budget(eng, copies, head_in_flight, spec_in_flight):
    """The header kernel's NUL searches pay into the sizing pass's counter, 4 KiB at a time, and are given up once the
    budget is spent; the real chain's headers are then read in frontier rounds.  copies: at most 16383 (one stored
    block); head_in_flight(candidates): the waves of the header kernel that run at a time, spec_in_flight likewise the
    sizing pass's workgroups -- the two kernels run one after the other and overshoot by a look's worth each."""
    image = nameless_image(copies)
    budget = 256 * 1024
    candidates, spec_bytes, rounds = check(eng, [image], budget, sound=True)
    free = sum(4 * (copies - j) for j in range(copies))  # what the searches read when nothing stops them
    slack = head_in_flight(candidates) * NUL_STRIDE + spec_in_flight(candidates) * SUPER
    print("nameless: %d candidates, %d bytes paid (budget %d, slack %d, unbudgeted NUL searches alone %d), %d frontier rounds" %
          (candidates, spec_bytes, budget, slack, free, rounds))
    assert candidates >= copies + 2
    assert budget <= spec_bytes <= budget + slack
    assert spec_bytes * 3 < free and (budget + slack) * 3 < free
    assert rounds > 0
    check(eng, [image], None, sound=True)
    check(eng, [image], 0, sound=True)


# ---------------------------------------------------------------------------
# the cases as files, for the sanitized stand-alone program (tests/gzip_main.cpp)
# ---------------------------------------------------------------------------
MEMBER_STRUCT = struct.Struct("<QQQQQIIIBBBBIIIIII")  # zh_gzip_member


def pack_members(recs):
    return b"".join(MEMBER_STRUCT.pack(r["coff"], r["cdata_off"], r["cdata_len"], r["uoff"], r["ulen"], r["crc"], r["isize"],
                                       r["mtime"], r["flg"], r["xfl"], r["os"], 0, r["extra_off"], r["extra_len"],
                                       r["name_off"], r["name_len"], r["comment_off"], r["comment_len"]) for r in recs)


def dump(out_dir):
    """cases.txt: "NAME IMAGES BUDGET" a line (BUDGET -1: none); NAME_<i>.bin image i, .out its data, .mem its members
    as zh_gzip_member records; NAME.st: a status a line (-1: any status but ZH_OK -- a stream zlib refuses).
    -> (cases, images)"""
    os.makedirs(out_dir, exist_ok=True)
    crafted = crafted_streams()
    ms = [member(pattern(400 + 50 * i, i), level=(1, 6, 9)[i % 3]) for i in range(5)]
    whole = b"".join(ms)
    inner = member(pattern(700, 4), name=b"inner.txt")
    sets = {
        "chains": [b"".join(members(k, seed=k)) for k in (0, 1, 2, 3, 64, 65)],
        "ends": [member(plain, raw=raw) + member(b"tail") for _, _, raw, plain in crafted[::3]] + [member(b"") * 3],
        "headers": [member(pattern(300, f), extra=b"ab\x03\x00xyz" if f & 1 else None, name=b"n" * (63 + f) if f & 2 else None,
                           comment=b"c" * 4097 if f & 4 else None, hcrc=bool(f & 8)) + member(b"next") for f in range(16)] +
                   [member(b"x", name=b"n", hcrc=True, hcrc_xor=0x100)],
        "false": [stored_member(inner) + ms[0], stored_member(b"\x1f\x8b\x08\x08" + b"no NUL " * 9) + ms[1],
                  stored_member(b"\x1f\x8b\x08\x00" + random.Random(5).randbytes(400))],
        "tails": [whole + b"\0" * 511, whole + b"\x01", whole + b"\x1f\x8b\x07" + b"\0" * 15, b"\0" * 18, whole[:-1],
                  whole[:-9], whole[:-12], b"".join([ms[0], member(b"abc", crc=5), ms[2]]), whole],
        "straddling": straddling_images()[0],
    }
    n_cases = n_images = 0
    with open(os.path.join(out_dir, "cases.txt"), "w") as listing:
        for name, images in sets.items():
            for budget in (-1, 0):
                case = "%s_b%d" % (name, budget + 1)
                listing.write("%s %d %d\n" % (case, len(images), budget))
                with open(os.path.join(out_dir, case + ".st"), "w") as stf:
                    for i, im in enumerate(images):
                        st, data, recs = gm.read(im, lambda src: -1)
                        stf.write("%d\n" % st)
                        base = os.path.join(out_dir, "%s_%d" % (case, i))
                        open(base + ".bin", "wb").write(im)
                        open(base + ".out", "wb").write(data or b"")
                        open(base + ".mem", "wb").write(pack_members(recs or []))
                n_cases += 1
                n_images += len(images)
        # the budgeted route proper: candidates that read on, a budget they exhaust, frontier rounds for the real chain
        image = stored_member((b"\x1f\x8b\x08\x00" + b"\0" * 6 + b"\x00\xff\xff\x00\x00" + b"A" * 100) * 60) + whole
        st, data, recs = gm.read(image, lambda src: -1)
        assert st == gm.OK
        listing.write("budgeted 1 4096\n")
        open(os.path.join(out_dir, "budgeted.st"), "w").write("0\n")
        open(os.path.join(out_dir, "budgeted_0.bin"), "wb").write(image)
        open(os.path.join(out_dir, "budgeted_0.out"), "wb").write(data)
        open(os.path.join(out_dir, "budgeted_0.mem"), "wb").write(pack_members(recs))
        # ... and names without an end: NUL searches that exhaust the budget, headers read in frontier rounds
        image = nameless_image(4096)
        st, data, recs = gm.read(image, lambda src: -1)
        assert st == gm.OK
        listing.write("nameless 1 8192\n")
        open(os.path.join(out_dir, "nameless.st"), "w").write("0\n")
        open(os.path.join(out_dir, "nameless_0.bin"), "wb").write(image)
        open(os.path.join(out_dir, "nameless_0.out"), "wb").write(data)
        open(os.path.join(out_dir, "nameless_0.mem"), "wb").write(pack_members(recs))
    return n_cases + 2, n_images + 2


# ---------------------------------------------------------------------------
# the interface
# ---------------------------------------------------------------------------
def check_interface(eng):
    import ctypes as c
    lib, h = eng.lib, eng._h
    image = b"".join(members(3, seed=2))
    assert eng.gzip_read_batch([]) == ([], [], [])
    assert eng.gzip_read_batch([], want_data=False, want_members=False) == ([], [], None)
    outs, sts, mems = eng.gzip_read_batch([image], want_members=False)
    assert sts == [0] and mems is None and outs[0] == gm.read(image, None)[1]
    srcs = (c.c_void_p * 1)(c.cast(c.c_char_p(image), c.c_void_p))
    lens = (c.c_size_t * 1)(len(image))
    sts = (c.c_int32 * 1)()
    dsts, dlens = (c.c_void_p * 1)(), (c.c_size_t * 1)()
    assert lib.zh_gzip_read_batch(h, None, lens, 1, dsts, dlens, sts, None, None) == 22
    assert lib.zh_gzip_read_batch(h, srcs, None, 1, dsts, dlens, sts, None, None) == 22
    assert lib.zh_gzip_read_batch(h, srcs, lens, 1, dsts, dlens, None, None, None) == 22
    assert lib.zh_gzip_read_batch(h, srcs, lens, 1, dsts, None, sts, None, None) == 22
    assert lib.zh_gzip_read_batch(None, srcs, lens, 1, dsts, dlens, sts, None, None) == 22
    assert lib.zh_gzip_read_batch(h, srcs, lens, 1, None, None, sts, None, None) == 0 and sts[0] == 0
    assert lib.zh_gzip_read_batch(h, None, None, 0, None, None, None, None, None) == 0


def check_api(eng, api):
    a, b = pattern(5000, 1), pattern(300, 2)
    image = member(a, name=b"a.txt") + member(b, comment=b"second", hcrc=True)
    assert api.gzip_read(image) == a + b
    recs = api.gzip_members(image)
    assert [r["ulen"] for r in recs] == [len(a), len(b)] and recs[1]["uoff"] == len(a)
    assert image[recs[0]["name_off"]:recs[0]["name_off"] + recs[0]["name_len"]] == b"a.txt"
    outs, sts, mems = api.gzip_read_batch([image, image[:-3], b""])
    assert sts[0] == 0 and sts[1] != 0 and sts[2] == 0 and outs == [a + b, None, b""] and mems[1] is None and mems[2] == []
    import pytest
    from zippy_amd.common import ZippyError
    with pytest.raises(ZippyError):
        api.gzip_read(image[:-3])
