"""Host-side mirror of the reference interface for the hot path (src/zippy.nim):

    compress(src, level=DefaultCompression, dataFormat=dfGzip) -> bytes     zippy.nim:11-16,86-98
    uncompress(src, dataFormat=dfDetect) -> bytes                          zippy.nim:100-104,167-177
    crc32(src) / adler32(src)                                              crc.nim:53,74 / adler32.nim:6,65

plus the batch forms the engine is built for.  Same names, argument meaning and
error behaviour (ZippyError) as the reference; every call goes through the C ABI
in include/zippy_hip.h into the gfx950 kernels.  No CPU fallback: importing this
module without the built library, or without a usable GPU, raises.
"""
import os

from ._binding import Engine
from .common import (ZippyError, dfDetect, dfZlib, dfGzip, dfDeflate, NoCompression, BestSpeed,
                     BestCompression, DefaultCompression, HuffmanOnly, TAR_PLAIN, tfDetect, tfUncompressed, tfGzip,
                     to_msdos)

# ZIPPY_HIP_LIB: tuning builds of the same library (tools/); never a different implementation
LIB_PATH = os.environ.get("ZIPPY_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                         "libzippy_hip.so")

_engine = None


def engine():
    global _engine
    if _engine is None:
        _engine = Engine(LIB_PATH)
    return _engine


def compress(src, level=DefaultCompression, dataFormat=dfGzip):
    return engine().compress(src, level, dataFormat)


def uncompress(src, dataFormat=dfDetect):
    return engine().uncompress(src, dataFormat)


def compress_batch(bufs, level=DefaultCompression, dataFormat=dfGzip):
    """n independent compress() calls in one launch sequence -> (outputs, statuses)."""
    return engine().compress_batch(bufs, level, dataFormat)


def uncompress_batch(bufs, dataFormat=dfDetect):
    return engine().uncompress_batch(bufs, dataFormat)


def compress_blocks(src, level=DefaultCompression, dataFormat=dfGzip, block_bytes=32768):
    """compress() with deflate blocks of block_bytes instead of deflate.nim:228's 4 MiB, plus the
    index of block starts; the stream still round-trips through zippy's uncompress()."""
    return engine().compress_blocks(src, level, dataFormat, block_bytes)


def uncompress_indexed(src, index, dataFormat=dfDetect):
    """uncompress() of a stream whose block index is known: one decoder per block."""
    return engine().uncompress_indexed(src, index, dataFormat)


def uncompress_ranges(streams, indexes, ranges):
    """Random access into streams written by compress_blocks: bytes [off, off + len) of the uncompressed data of
    streams[stream] for every (stream, off, len) of `ranges`, in one call -- only the blocks a range touches are
    uploaded and decoded.  Ranges read like pread (clipped at the end, empty beyond it).  -> (outputs, statuses);
    an output is None where its status is not 0."""
    return engine().uncompress_ranges(streams, indexes, ranges)


def read_range(src, index, off, length):
    """uncompress_ranges for one range of one stream -> bytes; raises ZippyError where the range cannot be read."""
    eng = engine()
    outs, sts = eng.uncompress_ranges([src], [index], [(0, off, length)])
    return eng._raise_first(outs, sts)[0]


def bgzf_compress_batch(srcs, level=DefaultCompression, block_bytes=0):
    """One BGZF file (the blocked gzip of bgzip / htslib: any gunzip reads it) per buffer, in one call: members of
    block_bytes (0: 65280) uncompressed bytes each and the EOF marker.  -> (outputs, statuses)"""
    return engine().bgzf_compress_batch(srcs, level, block_bytes)


def bgzf_compress(src, level=DefaultCompression, block_bytes=0):
    """bgzf_compress_batch for one buffer -> bytes; raises ZippyError."""
    eng = engine()
    outs, sts = eng.bgzf_compress_batch([src], level, block_bytes)
    return eng._raise_first(outs, sts)[0]


def bgzf_uncompress_batch(images):
    """The uncompressed data of BGZF files, every member verified by its CRC-32 and ISIZE.  -> (outputs, statuses); an
    output is None where its status is not 0."""
    return engine().bgzf_uncompress_batch(images)


def bgzf_uncompress(image):
    """bgzf_uncompress_batch for one file -> bytes; raises ZippyError."""
    eng = engine()
    outs, sts = eng.bgzf_uncompress_batch([image])
    return eng._raise_first(outs, sts)[0]


def bgzf_index(image):
    """The members of a BGZF file from its headers and trailers alone: [(coff, uoff), ...], closed by (the file's end,
    the uncompressed total).  Raises ZippyError where the file cannot be walked."""
    eng = engine()
    idx, sts, _ = eng.bgzf_index_batch([image])
    return eng._raise_first(idx, sts)[0]


def bgzf_read_ranges(images, indexes, ranges):
    """Random access into BGZF files: bytes [off, off + len) of the uncompressed data of images[image] for every
    (image, off, len) of `ranges`, in one call -- only the members a range touches are uploaded and decoded, each
    verified by its checksum.  Ranges read like pread.  -> (outputs, statuses); an output is None where its status is
    not 0."""
    return engine().bgzf_read_ranges(images, indexes, ranges)


def bgzf_read_range(image, index, off, length):
    """bgzf_read_ranges for one range of one file -> bytes; raises ZippyError where the range cannot be read."""
    eng = engine()
    outs, sts = eng.bgzf_read_ranges([image], [index], [(0, off, length)])
    return eng._raise_first(outs, sts)[0]


def gzip_read_batch(images, want_data=True):
    """Gzip files of any shape -- several members back to back (cat a.gz b.gz, appended logs, pigz -i, .warc.gz), FEXTRA,
    FNAME, FCOMMENT and FHCRC fields --, in one call; every member verified by its CRC-32 and ISIZE.  -> (outputs,
    statuses, members): an output is the members' data back to back (None where the status is not 0, and everywhere
    with want_data=False, which still decodes and verifies); members[i] is the list of image i's members as dicts
    with zh_gzip_member's fields."""
    return engine().gzip_read_batch(images, want_data)


def gzip_read(image):
    """gzip_read_batch for one file -> bytes; raises ZippyError."""
    eng = engine()
    outs, sts, _ = eng.gzip_read_batch([image])
    return eng._raise_first(outs, sts)[0]


def gzip_members(image):
    """The members of one gzip file, decoded and verified, without its data -> list of dicts; raises ZippyError."""
    eng = engine()
    _, sts, members = eng.gzip_read_batch([image], want_data=False)
    return eng._raise_first(members, sts)[0]


def seek_index_batch(srcs, dataFormat=dfDetect, span=0, want_data=False):
    """Seek indexes for foreign deflate streams (zlib, gzip, raw; from zlib, pigz or this library), in one call: every
    stream is decoded and verified once, and at block boundaries at least `span` uncompressed bytes apart (0: 1 MiB, else
    at least 32768) the index keeps the bit position, the output position and the 32 KiB of output before it, with a
    CRC-32 per interval.  -> (indexes, statuses), with want_data (indexes, statuses, outputs); an index is a blob of
    bytes that may be stored, None where the stream's status is not 0."""
    return engine().seek_index_batch(srcs, dataFormat, span, want_data)


def seek_index(src, dataFormat=dfDetect, span=0):
    """seek_index_batch for one stream -> the blob; raises ZippyError where the stream does not decode."""
    eng = engine()
    blobs, sts = eng.seek_index_batch([src], dataFormat, span)
    return eng._raise_first(blobs, sts)[0]


def seek_read_ranges(streams, indexes, ranges):
    """Random access into streams with seek indexes: bytes [off, off + len) of the uncompressed data of
    streams[stream] for every (stream, off, len) of `ranges`, in one call -- only the intervals a range touches, and
    their windows, are uploaded and decoded, each verified by its CRC-32.  Ranges read like pread.
    -> (outputs, statuses); an output is None where its status is not 0."""
    return engine().seek_read_ranges(streams, indexes, ranges)


def seek_read_range(src, index, off, length):
    """seek_read_ranges for one range of one stream -> bytes; raises ZippyError where the range cannot be read."""
    eng = engine()
    outs, sts = eng.seek_read_ranges([src], [index], [(0, off, length)])
    return eng._raise_first(outs, sts)[0]


def uncompress_resume_batch(srcs, states=None, max_out=1 << 20, last=None, dataFormat=dfDetect):
    """One step of many streams whose bytes arrive in pieces (zlib, gzip, raw), in one call: every stream decodes as many
    whole deflate blocks as its input holds and max_out allows.  srcs[i]: the unconsumed tail of stream i and what arrived
    since; states[i]: the state its step before returned (None: a new stream); last[i]: no more input will come.
    -> (outputs, consumed, new_states, why, statuses); why: 0 done (trailer verified), 1 more input, 2 more room."""
    return engine().uncompress_resume_batch(srcs, states, max_out, last, dataFormat)


class Inflater:
    """One stream decoded as its bytes arrive: feed(chunk) -> the bytes of the deflate blocks that became whole.  It
    keeps the unconsumed tail and the state between calls, doubles its budget where a block outgrows max_out, and raises
    ZippyError where the stream is damaged -- with last=True also where it ends early.  The call that meets the damage
    returns nothing, the good blocks of the same chunk included: feed smaller chunks to get what was decodable before
    it.  .done: the trailer is verified; .unused: the bytes behind it."""

    def __init__(self, fmt=dfDetect, max_out=1 << 20):
        self.fmt, self.max_out = fmt, max_out
        self.state, self.tail, self.done = None, b"", False

    @property
    def unused(self):
        return self.tail

    def feed(self, chunk, last=False):
        self.tail += bytes(chunk)
        if self.done:
            return b""
        eng = engine()
        made = []
        while True:
            outs, used, states, why, sts = eng.uncompress_resume_batch([self.tail], [self.state], self.max_out,
                                                                       [last], self.fmt)
            eng._raise_first(outs, sts)
            made.append(outs[0])
            self.tail = self.tail[used[0]:]
            self.state = states[0]
            if why[0] == 2:  # a block larger than the budget
                if not outs[0]:
                    self.max_out *= 2
                continue
            self.done = why[0] == 0
            return b"".join(made)


def uncompress_chunks(chunks, dataFormat=dfDetect, max_out=1 << 20):
    """uncompress() of a stream that comes as an iterable of byte pieces: yields the data as its blocks become whole;
    raises ZippyError where the stream is damaged or ends early."""
    inf = Inflater(dataFormat, max_out)
    held = None
    for chunk in chunks:
        if held is not None:
            out = inf.feed(held)
            if out:
                yield out
        held = chunk
    out = inf.feed(held if held is not None else b"", last=True)
    if out:
        yield out


FLUSH_BLOCK, FLUSH_SYNC, FLUSH_FINISH = 0, 1, 2


def compress_stream_batch(srcs, states=None, flush=None, level=DefaultCompression, dataFormat=dfGzip, block_bytes=0):
    """One step of many streams that are compressed piece by piece (zlib, gzip, raw), in one call: every stream's piece
    becomes whole deflate blocks of its own, placed bit-exactly behind what the stream has made so far.  srcs[i]: the
    next piece of stream i; states[i]: the state its step before returned (None: a new stream, which takes level,
    dataFormat and block_bytes -- 0: 4 MiB -- from this call); flush[i]: FLUSH_BLOCK (the blocks, up to 7 bits held
    back), FLUSH_SYNC (the default: then an empty stored block, so that all that was fed decodes from all that was
    delivered), FLUSH_FINISH (the last block and the trailer; no state comes back).
    -> (outputs, new_states, statuses)."""
    return engine().compress_stream_batch(srcs, states, flush, level, dataFormat, block_bytes)


class Deflater:
    """One stream compressed as its bytes arrive: feed(piece) -> the compressed bytes so far, finish() -> the rest with
    the trailer.  Pieces that are multiples of block_bytes fed with FLUSH_BLOCK and finished give compress()'s own bytes
    (block_bytes 0) or compress_blocks()'s; any other cut gives a valid stream of the same data.  A piece starts without
    history: small pieces cost ratio.  Raises ZippyError where a call fails."""

    def __init__(self, level=DefaultCompression, dataFormat=dfGzip, block_bytes=0):
        self.level, self.fmt, self.block_bytes = level, dataFormat, block_bytes
        self.state, self.started, self.done = None, False, False

    def feed(self, piece, flush=FLUSH_SYNC):
        if self.done:
            raise ValueError("the stream is finished")
        eng = engine()
        outs, states, sts = eng.compress_stream_batch([piece], [self.state] if self.started else None, [flush],
                                                      self.level, self.fmt, self.block_bytes)
        eng._raise_first(outs, sts)
        self.state, self.started, self.done = states[0], True, flush == FLUSH_FINISH
        return outs[0]

    def finish(self, piece=b""):
        return self.feed(piece, FLUSH_FINISH)


def compress_chunks(chunks, level=DefaultCompression, dataFormat=dfGzip, block_bytes=0, flush=FLUSH_SYNC):
    """compress() of data that comes as an iterable of byte pieces: yields the stream as it is made, every piece flushed
    with `flush`, the last one finished; the twin of uncompress_chunks."""
    d = Deflater(level, dataFormat, block_bytes)
    held = None
    for chunk in chunks:
        if held is not None:
            out = d.feed(held, flush)
            if out:
                yield out
        held = chunk
    out = d.finish(held if held is not None else b"")
    if out:
        yield out


def openZipArchive(image):
    """ziparchives.nim:183 openZipArchive on the bytes of an archive -> reader with walk_files(),
    extract_file(path), extract_batch(indices)."""
    return engine().open_zip(image)


def openZipArchives(images):
    """openZipArchive + the extraction of extractAll for many archives in one call (zh_zip_open_all_batch): every
    directory walked, every entry decoded and verified on the device -> a list of readers, in order, with
    .entries, .contents(i), .entry_status(i).  Raises ZippyError on the first archive whose status is not zero."""
    eng = engine()
    readers, sts = eng.open_zips(images)
    return eng._raise_first(readers, sts)


def createZipArchive(entries, dos_time=0, dos_date=0):
    """ziparchives.nim:625-634 createZipArchive(OrderedTable): entries = ordered mapping / pairs."""
    return engine().create_zip(entries, dos_time, dos_date)


def createZipArchives(tables, dos_time=0, dos_date=0, level=BestSpeed):
    """createZipArchive(OrderedTable) for many tables in one call (zh_zip_create_batch) -> a list of bytes, in order.
    Raises ZippyError on the first archive that failed.  BestSpeed is the reference's level (ziparchives.nim:530)."""
    eng = engine()
    outs, sts = eng.create_zips(tables, dos_time, dos_date, level)
    return eng._raise_first(outs, sts)


def openTarball(image):
    """tarballs.nim:26-124 on the bytes of a .tar.gz / .tar -> reader with .entries, .contents(i)."""
    return engine().open_tar(image)


def openTarballs(images):
    """openTarball for many images in one call (zh_tar_open_batch): every .tar.gz decoded in one batch, every header
    walk on the device -> a list of readers, in order.  Raises ZippyError on the first image that failed."""
    eng = engine()
    readers, sts = eng.open_tars(images)
    return eng._raise_first(readers, sts)


def readTarballs(images, formats=None):
    """tarballs_v1.nim:66-157 Tarball.open for many images in one call (zh_tar_read_batch): every gzip image decoded
    and verified in one batch, every header walk on the device -> a list of readers, in order, whose .entries are the
    table's keys in the table's order ('0' files with mode, mtime and .contents(i); '5' directories with nothing).
    formats: tfDetect / tfUncompressed / tfGzip, one an image; None: all detect.  Raises ZippyError on the first image
    that failed."""
    eng = engine()
    readers, sts = eng.read_tars(images, formats)
    return eng._raise_first(readers, sts)


def writeTarball(entries, dataFormat=dfGzip, level=DefaultCompression):
    """tarballs_v1.nim:203-270 writeTarball without the file write -> the bytes of the .tar.gz (dfGzip) or .tar
    (TAR_PLAIN).  entries: ordered mapping / (path, value) pairs; a value is the contents, or (contents, kind, mtime)
    with kind '0' (file) / '5' (directory) and mtime the Unix time (defaults '0', 0)."""
    return engine().create_tar(entries, dataFormat, level)


def writeZipArchive(entries, level=DefaultCompression):
    """ziparchives_v1.nim:371-486 writeZipArchive without the file write -> the bytes of the archive.
    entries: ordered mapping / (path, value) pairs; a value is the contents, or (contents, is_directory, dos_time,
    dos_date) with the DOS time and date of toMsDos (to_msdos(unix_time)); defaults False, 0, 0."""
    return engine().write_zip(entries, level)


def readZipArchives(images):
    """ziparchives_v1.nim:105-349 ZipArchive.open for many images in one call (zh_zip_read_batch): every image walked
    from byte 0, every entry decoded and verified on the device -> a list of readers, in order, with .entries (the
    table's keys in insertion order), .contents(i), .entry_v1(i).  Raises ZippyError on the first image that failed."""
    eng = engine()
    readers, sts = eng.read_zips(images)
    return eng._raise_first(readers, sts)


def crc32(src):
    return engine().crc32(src)


def adler32(src):
    return engine().adler32(src)
