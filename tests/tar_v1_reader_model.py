"""Tarball.open of the reference (src/zippy/tarballs_v1.nim:66-157 openStreamImpl), restated statement for statement
in Python: the referee of zh_tar_read_batch.  The decoder is the oracle's (uncompress(.., dfGzip)); a decoder failure
is carried as "the status zh_uncompress_batch gives for these bytes".  initTime(mtime, 0) and parseFilePermissions(mode)
(:147-148) are left out, as in the library: the numbers are kept.

No Nim toolchain or stdlib source is at hand: parse_oct_int and join restate std/parseutils.parseOct /
strutils.parseOctInt and std/os `/` as documented for Nim 1.4-2.x --
  parseOct(s, number): an optional 0o / 0O prefix, taken only when `i < s.len - 2` (a byte follows it); then '_' is
    skipped and '0'..'7' accumulate (number = number shl 3 or digit); the first other byte stops the scan; the result
    is the number of bytes consumed, 0 when no digit was seen;
  parseOctInt(s): ValueError unless parseOct consumed all of s and that is not 0;
  `/`: oracle/tar_oracle.py's _join, the join zh_tar_parse_kernel makes for tarballs.nim."""
from collections import OrderedDict

import oracle
from oracle.tar_oracle import _join as join

OK, TAR_FORMAT, TAR_OPEN, TAR_OPEN_MODE, TAR_EOF = 0, 46, 47, 48, 49
TF_DETECT, TF_UNCOMPRESSED, TF_GZIP = 0, 1, 2                            # :18-19


class Stop(Exception):
    """a raise site of openStreamImpl.  status: the library's code, or None when the failure is the decoder's (the
    library reports what zh_uncompress_batch says of the same bytes); decoder: the oracle's own code then"""

    def __init__(self, status, decoder=None):
        Exception.__init__(self, status)
        self.status, self.decoder = status, decoder


def parse_oct_int(s):
    """strutils.parseOctInt; ValueError as there"""
    i = 0
    if i < len(s) - 2 and s[i:i + 1] == b"0" and s[i + 1:i + 2] in (b"o", b"O"):
        i += 2
    number, found_digit = 0, False
    while i < len(s):
        c = s[i]
        if 0x30 <= c <= 0x37:
            number = (number << 3) | (c - 0x30)
            found_digit = True
        elif c == 0x5F:
            pass
        else:
            break
        i += 1
    consumed = i if found_digit else 0
    if consumed != len(s) or consumed == 0:
        raise ValueError("invalid oct integer: %r" % s)
    return number


def trim(s):                                                             # :71-75
    for i in range(len(s)):
        if s[i] == 0:
            return s[:i]
    return s


def walk(data):
    """the loop of :98-157 -> (table, counts); counts: headers, nameless, skipped (named headers of other types)"""
    contents = OrderedDict()
    counts = dict(headers=0, nameless=0, skipped=0)
    pos = 0                                                              # :98
    while pos < len(data):                                               # :99
        if pos + 512 > len(data):                                        # :100
            raise Stop(TAR_EOF)
        header = data[pos:pos + 512]                                     # :104
        file_name = trim(header[0:100])                                  # :105
        pos += 512                                                       # :107
        counts["headers"] += 1
        if len(file_name) == 0:                                          # :109
            counts["nameless"] += 1
            continue
        try:
            file_size = parse_oct_int(header[124:135])                   # :115
        except ValueError:
            raise Stop(TAR_OPEN)                                         # :118
        try:
            last_modified = parse_oct_int(header[136:147])               # :121
        except ValueError:
            raise Stop(TAR_OPEN)                                         # :124
        type_flag = header[156]                                          # :126
        try:
            file_mode = parse_oct_int(header[100:106])                   # :128
        except ValueError:
            raise Stop(TAR_OPEN_MODE)                                    # :131
        if header[257:263] == b"ustar\0":                                # :134
            file_name_prefix = trim(header[345:500])
        else:
            file_name_prefix = b""
        if pos + file_size > len(data):                                  # :139
            raise Stop(TAR_EOF)
        key = join(file_name_prefix, file_name).replace(b"\\", b"/")     # toUnixPath
        if type_flag in (0x30, 0):                                       # :142
            contents[key] = dict(kind=b"0", contents=data[pos:pos + file_size], mtime=last_modified,
                                 mode=file_mode & 0xFFFFFFFF, offset=pos, size=file_size)
        elif type_flag == 0x35:                                          # :150
            contents[key] = dict(kind=b"5", contents=b"", mtime=0, mode=0, offset=0, size=0)
        else:
            counts["skipped"] += 1
        pos += (file_size + 511) & ~511                                  # :157
    return contents, counts


def open_stream(data, tarball_format=TF_DETECT):
    """-> (the uncompressed image, the table: OrderedDict key -> dict(kind, contents, mtime, mode, offset, size), the
    counts); raises Stop"""
    data = bytes(data)
    if tarball_format == TF_DETECT:                                      # :80
        # (data[0], data[1] past the string are a Defect in the reference; the library: TAR_FORMAT)
        if len(data) == 0 or (data[0] == 0x1F and len(data) < 2):
            raise Stop(TAR_FORMAT)
        if data[0] == 0x1F:                                              # :81
            if data[1] == 0x8B:                                          # :83
                tarball_format = TF_GZIP
            else:
                raise Stop(TAR_FORMAT)                                   # :86
        else:
            tarball_format = TF_UNCOMPRESSED                             # :88
    if tarball_format == TF_GZIP:                                        # :93
        try:
            data = oracle.uncompress(data, oracle.dfGzip)                # :94
        except oracle.ZippyError as e:
            raise Stop(None, decoder=e.status)
    table, counts = walk(data)
    return data, table, counts


_cache = {}


def expected(image, tarball_format=TF_DETECT):
    """(status, uncompressed image | None, table | None); a decoder failure has status None (see Stop)"""
    key = (bytes(image), tarball_format)
    if key not in _cache:
        try:
            data, table, _ = open_stream(key[0], tarball_format)
            _cache[key] = (OK, data, table)
        except Stop as e:
            _cache[key] = (e.status, None, None)
    return _cache[key]
