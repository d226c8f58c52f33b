"""The contract of zh_compress_stream_batch (include/zippy_hip.h, "what the bytes are") in plain Python over the CPU
oracle: oracle.compress_blocks for a piece's own raw-deflate stream R and its block index, oracle.compress for the
container's header, integer bit arithmetic for the placing, the 64-byte state included.  step() is one call of one
stream; every call can leave a record of the quantities the placing turns on -- the pending bits k it found, (p + 3)
mod 8 and the byte delta where R has a stored block, the residue in front of a sync marker, the bits it left pending --
so that the tests can tell which cases they reach.  Test infrastructure only."""
import functools
import struct
import zlib

import oracle

DF_ZLIB, DF_GZIP, DF_DEFLATE = 1, 2, 3
BLOCK, SYNC, FINISH = 0, 1, 2
OK, INVALID_BUFFER, ARGUMENT = 0, 13, 22
MAGIC = b"ZHCSTRM1"
VERSION = 1
DEFAULT_BLOCK = 4194304
# magic, version, data_format, level, block_bytes, phase, pend_bits, pend_byte, check, total_in, total_out, reserved
STATE = struct.Struct("<8sIIiIIIIIQQQ")


def pack_state(fmt, level, block_bytes, pend_bits, pend_byte, check, total_in, total_out, phase=1, version=VERSION,
               magic=MAGIC, reserved=0):
    return STATE.pack(magic, version, fmt, level, block_bytes, phase, pend_bits, pend_byte, check, total_in, total_out,
                      reserved)


class State:
    def __init__(self, blob):
        (self.magic, self.version, self.fmt, self.level, self.block_bytes, self.phase, self.pend_bits, self.pend_byte,
         self.check, self.total_in, self.total_out, self.reserved) = STATE.unpack(blob)


def state_sound(blob):
    if blob is None or len(blob) != STATE.size:
        return False
    s = State(blob)
    return (s.magic == MAGIC and s.version == VERSION and s.fmt in (DF_ZLIB, DF_GZIP, DF_DEFLATE)
            and -2 <= s.level <= 9 and 32768 <= s.block_bytes <= DEFAULT_BLOCK and s.block_bytes % 32768 == 0
            and s.phase == 1 and s.pend_bits <= 7 and s.pend_byte >> s.pend_bits == 0 and s.reserved == 0)


@functools.lru_cache(maxsize=4096)
def piece_stream(piece, level, block_bytes):
    """R and its index: the piece compressed by itself as raw deflate"""
    return oracle.compress_blocks(piece, level, oracle.dfDeflate, block_bytes)


@functools.lru_cache(maxsize=64)
def head(level, fmt, fname_len):
    whole = oracle.compress(b"", level, fmt, fname_len)
    return whole[:11 + fname_len] if fmt == DF_GZIP else whole[:2] if fmt == DF_ZLIB else b""


def place(k, pend_byte, R, entries, final, rec):
    """the pending bits and, behind them, the bits [0, end) of R -> (the bit string as an integer, its length)"""
    end = entries[-1][0]
    r = int.from_bytes(R, "little") & ((1 << end) - 1)
    if not final:
        r &= ~(1 << entries[-2][0])  # BFINAL of the last block
    stored = [b for b, _ in entries[:-1] if (r >> (b + 1)) & 3 == 0]
    if not stored:
        return pend_byte | (r << k), end + k
    p = stored[0]
    seam_s, seam_d = (p + 3 + 7) // 8, (p + k + 3 + 7) // 8
    rec.update(p3=(p + 3) % 8, delta=seam_d - seam_s)
    assert seam_d - seam_s in (0, 1)
    low = r & ((1 << (p + 3)) - 1)
    return pend_byte | (low << k) | ((r >> (8 * seam_s)) << (8 * seam_d)), end - 8 * seam_s + 8 * seam_d


def step(state, piece, flush, level=oracle.DefaultCompression, fmt=DF_GZIP, block_bytes=0, fname_len=0, record=None):
    """one call of one stream -> (output, new state or None, status)"""
    piece = bytes(piece)
    rec = {}
    out = b""
    if state is None:
        s = State(pack_state(fmt, level, block_bytes or DEFAULT_BLOCK, 0, 0, 1 if fmt == DF_ZLIB else 0, 0, 0))
        out = head(level, fmt, fname_len)
    else:
        if not state_sound(state):
            return b"", None, INVALID_BUFFER
        s = State(state)
    rec["k"] = s.pend_bits
    val, nbits = s.pend_byte, s.pend_bits
    if piece or flush == FINISH:
        R, entries = piece_stream(piece, s.level, s.block_bytes)
        val, nbits = place(s.pend_bits, s.pend_byte, R, entries, flush == FINISH, rec)
    if flush == SYNC:
        rec["residue"] = nbits % 8
        nbits = (nbits + 3 + 7) // 8 * 8 + 32
        val |= 0xffff << (nbits - 16)
    elif flush == FINISH:
        nbits = (nbits + 7) // 8 * 8
    whole = nbits // 8
    out += (val & ((1 << (8 * whole)) - 1)).to_bytes(whole, "little")
    s.pend_bits, s.pend_byte = nbits % 8, val >> (8 * whole)
    assert s.pend_byte >> s.pend_bits == 0
    rec["pend"] = s.pend_bits
    if s.fmt == DF_GZIP:
        s.check = zlib.crc32(piece, s.check)
    elif s.fmt == DF_ZLIB:
        s.check = zlib.adler32(piece, s.check)
    s.total_in += len(piece)
    if flush == FINISH:
        if s.fmt == DF_GZIP:
            out += struct.pack("<II", s.check, s.total_in & 0xffffffff)
        elif s.fmt == DF_ZLIB:
            out += struct.pack(">I", s.check)
    s.total_out += len(out)
    if record is not None:
        record.append(rec)
    if flush == FINISH:
        return out, None, OK
    return out, pack_state(s.fmt, s.level, s.block_bytes, s.pend_bits, s.pend_byte, s.check, s.total_in, s.total_out), OK


def run(pieces, flushes, level=oracle.DefaultCompression, fmt=DF_GZIP, block_bytes=0, fname_len=0, record=None):
    """a whole stream: pieces[j] fed with flushes[j] -> the outputs of the calls"""
    state, outs = None, []
    for piece, fl in zip(pieces, flushes):
        out, state, st = step(state, piece, fl, level, fmt, block_bytes, fname_len, record)
        assert st == OK
        outs.append(out)
    return outs
