"""TEST INFRASTRUCTURE ONLY -- createZipArchive's framing (src/zippy/ziparchives.nim:541-624) restated for any level,
and the per-archive statuses of zh_zip_create_batch (include/zippy_hip.h).  The expected bytes of the tests are
oracle.zip_oracle.create_archive; this helper exists for what that function does not take -- a level other than
BestSpeed, a DOS time of an entry's own, streams from elsewhere -- and tests/test_emu_zip_create_batch.py holds it
equal to create_archive at level 1.  Never imported by zippy_amd."""
import struct

ZH_ERR_ARGUMENT, ZH_ERR_ZIP_DUPLICATE, ZH_ERR_ZIP_NAME = 22, 31, 33


class ZipCreateError(Exception):
    def __init__(self, status):
        Exception.__init__(self, status)
        self.status = status


def normalize(entries, dos_time=0, dos_date=0):
    """ordered mapping / pairs; value = contents or (contents, dos_time, dos_date) -> [(path, contents, time, date)]"""
    out = []
    for path, v in (entries.items() if hasattr(entries, "items") else entries):
        contents, t, d = v if isinstance(v, tuple) else (v, dos_time, dos_date)
        p = path.encode("utf-8", "surrogateescape") if isinstance(path, str) else bytes(path)
        out.append((p, contents, int(t), int(d)))
    return out


def check(entries):
    """the statuses before compression: entry by entry, last to first, the first failure wins -> 0 or the status"""
    seen = set()
    for path, _, _, _ in reversed(entries):
        if path == b"" or path[:1] == b"/" or len(path) > 0xFFFF:
            return ZH_ERR_ZIP_NAME
        if path in seen:
            return ZH_ERR_ZIP_DUPLICATE
        seen.add(path)
    return 0


def image(entries, dos_time=0, dos_date=0, level=1, deflate=None, crc32=None):
    """createZipArchive's bytes with compress(contents, level, dfDeflate) as the streams; raises
    ZipCreateError(status) where the library fails.  deflate(contents, level) -> the raw deflate stream (default: the
    oracle's); crc32(contents) (default: zlib's)."""
    entries = normalize(entries, dos_time, dos_date)
    st = check(entries)
    if st:
        raise ZipCreateError(st)
    if deflate is None:
        import oracle
        deflate = lambda c, lv: oracle.compress(c, lv, oracle.dfDeflate)  # noqa: E731
    if crc32 is None:
        import zlib
        crc32 = zlib.crc32
    out = bytearray()
    records = []
    for path, contents, t, d in reversed(entries):  # :503-566
        contents = bytes(contents)
        method = 8 if contents else 0
        crc = crc32(contents) if contents else 0
        comp = deflate(contents, level) if contents else b""
        records.append((path, len(out), len(contents), len(comp), method, crc, t, d))
        out += struct.pack("<IHHHHHIIIHH", 0x04034B50, 45, 0x0800, method, t, d, crc, 0xFFFFFFFF, 0xFFFFFFFF,
                           len(path), 20)
        out += path
        out += struct.pack("<HHQQ", 1, 16, len(contents), len(comp))
        out += comp
    cd_start = len(out)
    for path, hoff, ulen, clen, method, crc, t, d in records:  # :570-596
        out += struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 45, 45, 0x0800, method, t, d, crc, 0xFFFFFFFF,
                           0xFFFFFFFF, len(path), 28, 0, 0, 0, 0, 0xFFFFFFFF)
        out += path
        out += struct.pack("<HHQQQ", 1, 24, ulen, clen, hoff)
    cd_end = len(out)
    out += struct.pack("<IQHHIIQQQQ", 0x06064B50, 44, 45, 45, 0, 0, len(records), len(records), cd_end - cd_start,
                       cd_start)  # :600-609
    out += struct.pack("<IIQI", 0x07064B50, 0, cd_end, 1)  # :611-614
    out += struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, 0xFFFF, 0xFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0)  # :616-623
    return bytes(out)


def status(entries):
    return check(normalize(entries))


def framing(img):
    """an archive's bytes with every stream cut out and every compressed length zeroed -> (bytes, [stream, ...]):
    what two archives of the same entries share whatever their deflate streams are"""
    img = bytearray(img)
    out, streams, pos = bytearray(), [], 0
    while img[pos:pos + 4] == b"PK\x03\x04":
        plen = struct.unpack_from("<H", img, pos + 26)[0]
        extra = pos + 30 + plen
        clen = struct.unpack_from("<Q", img, extra + 12)[0]
        out += img[pos:extra + 12] + bytes(8)
        streams.append(bytes(img[extra + 20:extra + 20 + clen]))
        pos = extra + 20 + clen
    cd_start = pos
    while img[pos:pos + 4] == b"PK\x01\x02":
        plen = struct.unpack_from("<H", img, pos + 28)[0]
        extra = pos + 46 + plen
        out += img[pos:extra + 12] + bytes(16)  # (the compressed length and the header's offset, which follows from them)
        pos = extra + 28
    assert img[pos:pos + 4] == b"PK\x06\x06" and len(img) == pos + 98
    assert struct.unpack_from("<QQ", img, pos + 40) == (pos - cd_start, cd_start)
    assert struct.unpack_from("<Q", img, pos + 64)[0] == pos
    out += img[pos:pos + 40] + bytes(16) + img[pos + 56:pos + 64] + bytes(8) + img[pos + 72:]
    return bytes(out), streams
