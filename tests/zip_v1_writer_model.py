"""TEST INFRASTRUCTURE ONLY -- a Python restatement of writeZipArchive (src/zippy/ziparchives_v1.nim:371-486: the
bytes) and of the checks zh_zip_write_batch adds where the reference has no answer (include/zippy_hip.h).  The deflate
streams come from the CPU oracle's compress(contents, level, dfDeflate).  Never imported by zippy_amd."""
import struct

ZH_ERR_ARGUMENT, ZH_ERR_ZIP_DUPLICATE, ZH_ERR_ZIP_EMPTY, ZH_ERR_ZIP_TOO_LARGE = 22, 31, 40, 41
LIMIT32 = 1 << 32


class ZipWriteError(Exception):
    def __init__(self, status):
        Exception.__init__(self, status)
        self.status = status


def split_file_name(path):
    """std/os splitFile(path).name on POSIX ('/' is DirSep and AltSep, '.' ExtSep), line by line"""
    name_pos, dot_pos = 0, 0
    for i in range(len(path) - 1, -1, -1):
        c = path[i:i + 1]
        if c == b"/" or i == 0:
            if c == b"/":
                name_pos = i + 1
            if dot_pos > i:
                return path[name_pos:dot_pos]
            return path[name_pos:]
        if c == b"." and 0 < i < len(path) - 1 and path[i - 1:i] != b"/" and path[i + 1:i + 2] != b"." \
                and dot_pos == 0:
            dot_pos = i
    return b""


def stored(path):
    """method 0 by the path alone: splitFile(path).name is empty (ziparchives_v1.nim:393-396)"""
    return len(split_file_name(path)) == 0


def normalize(entries):
    """ordered mapping / pairs; value = contents or (contents, is_directory, dos_time, dos_date)
    -> [(path, contents, is_directory, dos_time, dos_date)]"""
    out = []
    for path, v in (entries.items() if hasattr(entries, "items") else entries):
        contents, is_dir, t, d = v, False, 0, 0
        if isinstance(v, tuple):
            contents, is_dir, t, d = v + (False, 0, 0)[len(v) - 1:]
        p = path.encode("utf-8", "surrogateescape") if isinstance(path, str) else bytes(path)
        out.append((p, contents, bool(is_dir), int(t), int(d)))
    return out


def check(entries):
    """steps 1-4 of the statuses -> 0 or the status"""
    if not entries:
        return ZH_ERR_ZIP_EMPTY
    if len(entries) > 0xFFFF:
        return ZH_ERR_ZIP_TOO_LARGE
    for path, contents, _, _, _ in entries:
        if len(path) > 0xFFFF or len(contents) >= LIMIT32:
            return ZH_ERR_ZIP_TOO_LARGE
    for path, contents, _, _, _ in entries:
        if len(contents) and stored(path):
            return ZH_ERR_ARGUMENT
    seen = set()
    for path, _, _, _, _ in entries:
        if path in seen:
            return ZH_ERR_ZIP_DUPLICATE
        seen.add(path)
    return 0


def image(entries, level=-1, limit=LIMIT32, deflate=None, crc32=None):
    """writeZipArchive's `data` at `level` (the reference: DefaultCompression); raises ZipWriteError(status) where
    the library fails.  deflate(contents, level) -> the raw deflate stream (default: the oracle's); crc32(contents)
    (default: zlib's)."""
    entries = normalize(entries)
    st = check(entries)
    if st:
        raise ZipWriteError(st)
    if deflate is None:
        import oracle
        deflate = lambda c, lv: oracle.compress(c, lv, oracle.dfDeflate)  # noqa: E731
    if crc32 is None:
        import zlib
        crc32 = zlib.crc32
    data = bytearray()
    values = []
    for path, contents, _, t, d in entries:  # :383-425
        offset = len(data)
        method = 0 if stored(path) or not contents else 8
        crc = crc32(contents) if contents else 0
        comp = deflate(contents, level) if contents else b""
        if len(comp) >= limit or offset >= limit:
            raise ZipWriteError(ZH_ERR_ZIP_TOO_LARGE)
        data += struct.pack("<IHHHHHIIIHH", 0x04034B50, 20, 0x0800, method, t, d, crc, len(comp), len(contents),
                            len(path), 0)
        data += path
        data += comp
        values.append((offset, crc, len(comp), len(contents), method))
    cd_offset = len(data)
    for (path, _, is_dir, t, d), (offset, crc, clen, ulen, method) in zip(entries, values):  # :427-467
        data += struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 63, 20, 0x0800, method, t, d, crc, clen, ulen,
                            len(path), 0, 0, 0, 0, 0x10 if is_dir else 0x20, offset)
        data += path
    cd_size = len(data) - cd_offset
    if cd_size >= limit or cd_offset >= limit:
        raise ZipWriteError(ZH_ERR_ZIP_TOO_LARGE)
    data += struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, len(entries), len(entries), cd_size, cd_offset, 0)  # :469-477
    return bytes(data)


def status(entries, level=-1, limit=LIMIT32):
    try:
        image(entries, level, limit)
    except ZipWriteError as e:
        return e.status
    return 0
