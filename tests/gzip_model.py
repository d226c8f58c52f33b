"""A plain-Python model of zh_gzip_read_batch (include/zippy_hip.h): a gzip image of any shape is walked member by
member with zlib.decompressobj(-15) and its unused_data, the header checks and the member verdict are applied in the
order the header states them, and what comes back is the image's status, its data and its member records.  Written
from RFC 1952 and the header comment, not from the device code.

Where zlib refuses a deflate stream (or runs out of input), the status to give is the codec's own for the same bytes:
`decoder_status(bytes) -> int`, which the caller supplies (tests/gzip_cases.py: Engine.uncompress_batch, raw deflate)."""
import struct
import zlib

OK = 0
UNSUPPORTED_METHOD, CHECKSUM, SIZE, GZIP_ID, RESERVED_FLAGS, INVALID_BUFFER = 4, 8, 9, 10, 11, 13

FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16
FIELDS = ("coff", "cdata_off", "cdata_len", "uoff", "ulen", "crc", "isize", "mtime", "flg", "xfl", "os",
          "extra_off", "extra_len", "name_off", "name_len", "comment_off", "comment_len")


def header_at(image, pos):
    """-> (status, record): the header checks of the member at `pos`, the first failure decides"""
    left = len(image) - pos
    q = image[pos:]
    if left < 18:
        return INVALID_BUFFER, None
    if q[0] != 0x1f or q[1] != 0x8b:
        return GZIP_ID, None
    if q[2] != 8:
        return UNSUPPORTED_METHOD, None
    flg = q[3]
    if flg & 0xe0:
        return RESERVED_FLAGS, None
    rec = dict.fromkeys(FIELDS, 0)
    rec.update(coff=pos, flg=flg, mtime=struct.unpack_from("<I", q, 4)[0], xfl=q[8], os=q[9])
    off = 10
    if flg & FEXTRA:
        xlen = struct.unpack_from("<H", q, 10)[0]
        if 12 + xlen > left:
            return INVALID_BUFFER, None
        rec.update(extra_off=12, extra_len=xlen)
        off = 12 + xlen
    for flag, name in ((FNAME, "name"), (FCOMMENT, "comment")):
        if flg & flag:
            z = q.find(b"\0", off)
            if z < 0:
                return INVALID_BUFFER, None
            rec[name + "_off"], rec[name + "_len"] = off, z - off
            off = z + 1
    rec["hcrc_off"] = 0
    if flg & FHCRC:
        if off + 2 > left:
            return INVALID_BUFFER, None
        rec["hcrc_off"] = off
        off += 2
    rec["cdata_off"] = pos + off
    return OK, rec


def read(image, decoder_status):
    """-> (status, data or None, members or None)"""
    image = bytes(image)
    n = len(image)
    pos, uoff, members, out = 0, 0, [], []
    while pos < n:
        if members and not any(image[pos:]):
            break  # zeros to the end: padding
        st, rec = header_at(image, pos)
        if st != OK:
            return st, None, None
        src = image[rec["cdata_off"]:max(rec["cdata_off"], n - 8)]
        d = zlib.decompressobj(-15)
        try:
            plain = d.decompress(src)
        except zlib.error:
            plain = None
        if plain is None or not d.eof:
            st = decoder_status(src)
            assert st != OK, "zlib refuses a stream the codec takes"
            return st, None, None
        clen = len(src) - len(d.unused_data)
        end = rec["cdata_off"] + clen + 8
        if end > n:
            return INVALID_BUFFER, None, None
        hcrc_off = rec.pop("hcrc_off")
        if hcrc_off and zlib.crc32(image[pos:pos + hcrc_off]) & 0xffff != struct.unpack_from("<H", image, pos + hcrc_off)[0]:
            return CHECKSUM, None, None
        crc, isize = struct.unpack_from("<II", image, end - 8)
        if zlib.crc32(plain) != crc:
            return CHECKSUM, None, None
        if len(plain) & 0xffffffff != isize:
            return SIZE, None, None
        rec.update(cdata_len=clen, uoff=uoff, ulen=len(plain), crc=crc, isize=isize)
        members.append(rec)
        out.append(plain)
        uoff += len(plain)
        pos = end
    return OK, b"".join(out), members
