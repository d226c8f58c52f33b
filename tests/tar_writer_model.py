"""TEST INFRASTRUCTURE ONLY -- a Python restatement of writeTarball (src/zippy/tarballs_v1.nim:203-261: the image)
and of the checks zh_tar_create_batch adds where the reference has no answer (include/zippy_hip.h).  Never imported
by zippy_amd."""

ZH_ERR_ARGUMENT, ZH_ERR_TAR_EMPTY, ZH_ERR_TAR_PATH, ZH_ERR_TAR_NAME = 22, 37, 38, 39
OCT11 = 8 ** 11


class TarWriteError(Exception):
    def __init__(self, status):
        Exception.__init__(self, status)
        self.status = status


def split_path(path):
    """std/os splitPath on POSIX: '/' only; head = path[:max(s, 1)], tail = path[s + 1:] (s: the last '/')."""
    s = path.rfind(b"/")
    if s < 0:
        return b"", path
    return path[:max(s, 1)], path[s + 1:]


def to_oct(x, n):  # std/strutils toOct: the low n octal digits, zero-padded
    return bytes(ord("0") + ((x >> (3 * (n - 1 - j))) & 7) for j in range(n))


def normalize(entries):
    """ordered mapping / pairs; value = contents or (contents, kind, mtime) -> [(path, contents, kind, mtime)]"""
    out = []
    for path, v in (entries.items() if hasattr(entries, "items") else entries):
        contents, kind, mtime = v, "0", 0
        if isinstance(v, tuple):
            contents, kind, mtime = v + ("0", 0)[len(v) - 1:]
        p = path.encode() if isinstance(path, str) else bytes(path)
        k = kind.encode("latin-1") if isinstance(kind, str) else bytes(kind)
        out.append((p, bytes(contents), k, int(mtime)))
    return out


def header(path, contents_len, kind, mtime):
    """the 512 bytes of tarballs_v1.nim:229-255"""
    head, tail = split_path(path)
    h = bytearray(512)
    h[0:len(tail)] = tail
    h[100:108] = b"000777 \0"
    h[108:116] = to_oct(0, 6) + b" \0"
    h[116:124] = to_oct(0, 6) + b" \0"
    h[124:136] = to_oct(contents_len, 11) + b" "
    h[136:148] = to_oct(mtime, 11) + b" "
    h[148:156] = b"        "
    h[156:157] = kind
    h[257:263] = b"ustar\0"
    h[263:265] = to_oct(0, 2)
    h[329:337] = to_oct(0, 6) + b"\0 "
    h[337:345] = to_oct(0, 6) + b"\0 "
    h[345:345 + len(head)] = head
    h[148:155] = to_oct(sum(h), 6) + b"\0"
    return bytes(h)


def check(entries):
    """-> 0, or the status zh_tar_create_batch gives this tarball"""
    if not entries:
        return ZH_ERR_TAR_EMPTY
    seen = set()
    for path, contents, kind, mtime in entries:
        head, tail = split_path(path)
        if len(head) >= 155:
            return ZH_ERR_TAR_PATH
        if len(tail) >= 100:
            return ZH_ERR_TAR_NAME
        if kind not in (b"0", b"5") or len(contents) >= OCT11 or not 0 <= mtime < OCT11 or path in seen:
            return ZH_ERR_ARGUMENT
        seen.add(path)
    return 0


def image(entries):
    """writeTarball's `data` (tarballs_v1.nim:209-261); raises TarWriteError(status) where the library fails"""
    entries = normalize(entries)
    st = check(entries)
    if st:
        raise TarWriteError(st)
    out = bytearray()
    for path, contents, kind, mtime in entries:
        out += header(path, len(contents), kind, mtime)
        out += contents
        out += bytes(-len(out) % 512)
    out += bytes(1024)
    return bytes(out)


def status(entries):
    return check(normalize(entries))
