"""BGZF (SAM specification, section 4.1) restated in plain Python, as include/zippy_hip.h describes zh_bgzf_*: the
writer from the oracle's raw deflate with the level-0 rule, the walk with its checks in their order, the whole-file
read, the index and the range reads.  The reference has no counterpart; the model is held against Python's own gzip
in tests/test_bgzf_model.py.

A decoder is a callable cdata -> (status, bytes); oracle_decoder is the reference's inflate."""
import struct
import zlib

import oracle

OK, UNSUPPORTED_METHOD, CHECKSUM, SIZE, GZIP_ID, RESERVED_FLAGS, UNSUPPORTED_FLAGS, INVALID_BUFFER = 0, 4, 8, 9, 10, 11, 12, 13
ARGUMENT, INVALID_LEVEL, BGZF_HEADER = 22, 1, 50
BLOCK, MAX_BLOCK, MAX_CDATA = 65280, 65505, 65510
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
HEADER = bytes.fromhex("1f8b08040000000000ff060042430200")


def member(cdata, crc, isize):
    """one member around a raw-deflate stream"""
    return HEADER + struct.pack("<H", 18 + len(cdata) + 8 - 1) + cdata + struct.pack("<II", crc & 0xFFFFFFFF, isize)


def cdata_of(piece, level):
    """the engine's raw deflate of a piece, or its level-0 form where that does not fit a member"""
    c = oracle.compress(piece, level, oracle.dfDeflate)
    if len(c) > MAX_CDATA:
        c = oracle.compress(piece, 0, oracle.dfDeflate)
        assert len(c) == 5 + len(piece) <= MAX_CDATA
    return c


def write(src, level, block_bytes=0):
    b = block_bytes or BLOCK
    assert 1 <= b <= MAX_BLOCK
    src = bytes(src)
    out = []
    for o in range(0, len(src), b):
        piece = src[o:o + b]
        out.append(member(cdata_of(piece, level), zlib.crc32(piece), len(piece)))
    return b"".join(out) + EOF


class Member:
    def __init__(self, coff):
        self.coff, self.status = coff, OK
        self.end = self.cdata_off = self.cdata_len = self.isize = self.crc = 0


def member_at(image, pos):
    """the checks of a member at pos, in their order: the first that fails is its status"""
    m = Member(pos)
    left = len(image) - pos
    q = image[pos:]

    def fail(st):
        m.status = st
        return m
    if left < 12:
        return fail(INVALID_BUFFER)
    if q[0] != 0x1F or q[1] != 0x8B:
        return fail(GZIP_ID)
    if q[2] != 8:
        return fail(UNSUPPORTED_METHOD)
    if q[3] & 0xE0:
        return fail(RESERVED_FLAGS)
    if q[3] != 4:
        return fail(UNSUPPORTED_FLAGS)
    xlen = q[10] | q[11] << 8
    if 12 + xlen > left:
        return fail(INVALID_BUFFER)
    o, bsize = 0, None
    while o < xlen:
        if o + 4 > xlen:
            return fail(BGZF_HEADER)
        slen = q[12 + o + 2] | q[12 + o + 3] << 8
        if o + 4 + slen > xlen:
            return fail(BGZF_HEADER)
        if bsize is None and q[12 + o] == 0x42 and q[12 + o + 1] == 0x43 and slen == 2:
            bsize = q[12 + o + 4] | q[12 + o + 5] << 8
        o += 4 + slen
    if bsize is None:
        return fail(BGZF_HEADER)
    total = bsize + 1
    if total < 12 + xlen + 8:
        return fail(BGZF_HEADER)
    if total > left:
        return fail(INVALID_BUFFER)
    m.end = pos + total
    m.cdata_off = pos + 12 + xlen
    m.cdata_len = total - 8 - 12 - xlen
    m.crc, m.isize = struct.unpack_from("<II", q, total - 8)
    if m.isize > 65536:
        return fail(BGZF_HEADER)
    return m


def walk(image):
    """-> (members reached in file order -- a last one may have failed --, has_eof).  The walk ends cleanly where a
    member ends with the image."""
    image = bytes(image)
    out, pos = [], 0
    while pos != len(image):
        m = member_at(image, pos)
        out.append(m)
        if m.status != OK:
            return out, 0
        pos = m.end
    return out, 1 if out and image[out[-1].coff:] == EOF else 0


def oracle_decoder(cdata):
    try:
        return OK, oracle.uncompress(cdata, oracle.dfDeflate)
    except oracle.ZippyError as e:
        return e.status, b""


def settle(image, m, decoder):
    """a member with a sound header -> (status, its bytes): the decoder's status (more bytes than ISIZE promises:
    SIZE), then the CRC-32, then the length"""
    st, data = decoder(image[m.cdata_off:m.cdata_off + m.cdata_len])
    if st != OK:
        return st, b""
    if len(data) > m.isize:
        return SIZE, b""
    if zlib.crc32(data) != m.crc:
        return CHECKSUM, b""
    if len(data) != m.isize:
        return SIZE, b""
    return OK, data


def read(image, decoder=oracle_decoder):
    """-> (status, data | None, has_eof): the first failing member in file order decides"""
    image = bytes(image)
    members, has_eof = walk(image)
    out = []
    for m in members:
        if m.status != OK:
            return m.status, None, has_eof
        st, data = settle(image, m, decoder)
        if st != OK:
            return st, None, has_eof
        out.append(data)
    return OK, b"".join(out), has_eof


def index(image):
    """-> (status, [(coff, uoff), ...] closed by (end of the walk, total) | None, has_eof)"""
    members, has_eof = walk(image)
    if members and members[-1].status != OK:
        return members[-1].status, None, has_eof
    entries, uoff = [], 0
    for m in members:
        entries.append((m.coff, uoff))
        uoff += m.isize
    entries.append((members[-1].end if members else 0, uoff))
    return OK, entries, has_eof


def index_sound(idx, image_len):
    if len(idx) < 1 or idx[0][1] != 0:
        return False
    for k, (coff, uoff) in enumerate(idx):
        if coff > image_len:
            return False
        if k + 1 < len(idx) and (idx[k + 1][0] < coff or idx[k + 1][1] < uoff or idx[k + 1][1] - uoff > 65536):
            return False
    return True


def touched(idx, off, length):
    """the clipped range and the members that hold a byte of it -> (off, end, [k, ...])"""
    total = idx[-1][1]
    if off >= total or not length:
        return 0, 0, []
    end = min(total, off + length)
    return off, end, [k for k in range(len(idx) - 1) if idx[k][1] < end and idx[k + 1][1] > off and idx[k + 1][1] > idx[k][1]]


def ranges(images, indexes, rngs, decoder=oracle_decoder):
    """-> ([bytes | None], [status]) like pread over the uncompressed data; every touched member is parsed where the
    index says it is, must end where the next begins and promise what the index promises, and is verified whole"""
    outs, sts = [], []
    for (t, off, length) in rngs:
        image, idx = bytes(images[t]), indexes[t]
        if not index_sound(idx, len(image)):
            outs.append(None)
            sts.append(INVALID_BUFFER)
            continue
        off, end, ks = touched(idx, off, length)
        parts, st = [], OK
        for k in ks:
            own = image[idx[k][0]:idx[k + 1][0]]
            m = member_at(own, 0)
            st = m.status
            if st == OK and (m.end != len(own) or m.isize != idx[k + 1][1] - idx[k][1]):
                st = INVALID_BUFFER
            if st == OK:
                st, data = settle(own, m, decoder)
            if st != OK:
                break
            parts.append(data[max(off, idx[k][1]) - idx[k][1]:min(end, idx[k + 1][1]) - idx[k][1]])
        outs.append(b"".join(parts) if st == OK else None)
        sts.append(st)
    return outs, sts
