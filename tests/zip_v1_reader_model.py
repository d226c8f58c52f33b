"""ZipArchive.open of the reference (src/zippy/ziparchives_v1.nim:105-329 openStreamImpl), restated statement for
statement in Python: the referee of zh_zip_read_batch.  The decoder and the CRC are the oracle's (uncompress(..,
dfDeflate), crc32).  The conversion of the DOS words to times.Time (:161-179) is left out, as in the library: the raw
words are kept."""
import struct
from collections import OrderedDict

import oracle

OK, ARCHIVE_EOF, METHOD, CRC = 0, 23, 25, 27
DATA_DESCRIPTOR, DEFLATE64, SIZE, OPEN = 42, 43, 44, 45


class Stop(Exception):
    """a raise site of openStreamImpl.  status: the library's code; decoder: the oracle's own code when the failure
    is the decoder's (the library reports what zh_uncompress_batch says of the same bytes), stream: those bytes"""

    def __init__(self, status, decoder=None, stream=None):
        Exception.__init__(self, status)
        self.status, self.decoder, self.stream = status, decoder, stream


def read16(data, pos):
    return struct.unpack_from("<H", data, pos)[0]


def read32(data, pos):
    return struct.unpack_from("<I", data, pos)[0]


def open_stream(data):
    """-> the table: OrderedDict key -> dict(contents, dos_time, dos_date, is_directory, unix_mode, in_directory,
    header_offset, compressed_size, uncompressed_size, crc32); raises Stop"""
    data = bytes(data)
    contents = OrderedDict()                                              # :108 archive.clear()
    pos = 0                                                               # :113
    while True:                                                           # :114
        if pos + 4 > len(data):                                           # :115
            raise Stop(ARCHIVE_EOF)
        signature = read32(data, pos)                                     # :118
        if signature == 0x04034B50:                                       # :120
            if pos + 30 > len(data):                                      # :121
                raise Stop(ARCHIVE_EOF)
            header_offset = pos
            flag = read16(data, pos + 6)                                  # :126
            method = read16(data, pos + 8)
            dos_time = read16(data, pos + 10)
            dos_date = read16(data, pos + 12)
            crc = read32(data, pos + 14)
            compressed_size = read32(data, pos + 18)
            uncompressed_size = read32(data, pos + 22)
            name_len = read16(data, pos + 26)
            extra_len = read16(data, pos + 28)
            pos += 30                                                     # :136
            if flag & 0b100:                                              # :138
                raise Stop(DATA_DESCRIPTOR)
            if flag & 0b1000:                                             # :144
                raise Stop(DEFLATE64)
            if method not in (0, 8):                                      # :181
                raise Stop(METHOD)
            if pos + name_len + extra_len > len(data):                    # :187
                raise Stop(ARCHIVE_EOF)
            name = data[pos:pos + name_len]                               # :190
            pos += name_len
            pos += extra_len                                              # :194
            if pos + compressed_size > len(data):                         # :199
                raise Stop(ARCHIVE_EOF)
            if method == 0:                                               # :202
                uncompressed = data[pos:pos + compressed_size]
            else:
                try:
                    uncompressed = oracle.uncompress(data[pos:pos + compressed_size], oracle.dfDeflate)
                except oracle.ZippyError as e:
                    raise Stop(None, decoder=e.status, stream=data[pos:pos + compressed_size])
            if oracle.crc32(uncompressed) != crc:                         # :208
                raise Stop(CRC)
            if len(uncompressed) != uncompressed_size:                    # :213
                raise Stop(SIZE)
            key = name.replace(b"\\", b"/")                               # :219 toUnixPath
            # (a fresh ArchiveEntry: kind ekFile, no permissions; an equal key keeps its place in the order)
            contents[key] = dict(contents=uncompressed, dos_time=dos_time, dos_date=dos_date, is_directory=False,
                                 unix_mode=0, in_directory=0, header_offset=header_offset,
                                 compressed_size=compressed_size, uncompressed_size=uncompressed_size, crc32=crc)
            pos += compressed_size                                        # :225
        elif signature == 0x02014B50:                                     # :227
            if pos + 46 > len(data):                                      # :228
                raise Stop(ARCHIVE_EOF)
            name_len = read16(data, pos + 28)                             # :241
            extra_len = read16(data, pos + 30)
            comment_len = read16(data, pos + 32)
            external = read32(data, pos + 38)
            pos += 46                                                     # :266
            if pos + name_len + extra_len + comment_len > len(data):      # :268
                raise Stop(ARCHIVE_EOF)
            name = data[pos:pos + name_len]                               # :271
            pos += name_len + extra_len + comment_len
            if name not in contents:                                      # :282-293 KeyError -> failOpen
                raise Stop(OPEN)
            if external & 0x10:                                           # :284
                contents[name]["is_directory"] = True
            contents[name]["unix_mode"] = external >> 16                  # :291 (extractPermissions' input)
            contents[name]["in_directory"] = 1
        elif signature == 0x06054B50:                                     # :295
            if pos + 22 > len(data):                                      # :296
                raise Stop(ARCHIVE_EOF)
            comment_len = read16(data, pos + 20)                          # :306
            pos += 22
            if pos + comment_len > len(data):                             # :318
                raise Stop(ARCHIVE_EOF)
            break                                                         # :326
        else:
            raise Stop(OPEN)                                              # :328
    return contents


_cache = {}


def expected(image):
    """(status, table | None, Stop | None); a decoder failure has status None (see Stop)"""
    image = bytes(image)
    if image not in _cache:
        try:
            _cache[image] = (OK, open_stream(image), None)
        except Stop as e:
            _cache[image] = (e.status, None, e)
    return _cache[image]
