## MI355X backend for zippy's compress()/uncompress() hot path -- the binding a maintainer drops into the
## reference tree as src/zippy/hip.nim (build with -d:zippyHip; see INTEGRATION.md, which quotes this file).
## Binds libzippy_hip.so (include/zippy_hip.h).  NOT compiled anywhere in this repository: the build image has no
## Nim.  tests/test_abi.py checks that every `importc` proc declared here names a symbol the header declares and
## the library exports, with the same number of parameters; the C99 consumer (tests/native/c_consumer.c) drives the
## same calls end to end.
import common

const zhLib = "libzippy_hip.so"

type
  ZhCtx = pointer

proc zh_create(device: cint, stream: pointer, ctx: ptr ZhCtx): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_destroy(ctx: ZhCtx) {.importc, cdecl, dynlib: zhLib.}
proc zh_strerror(status: cint): cstring {.importc, cdecl, dynlib: zhLib.}
proc zh_free(p: pointer) {.importc, cdecl, dynlib: zhLib.}
proc zh_compress(ctx: ZhCtx, src: pointer, len: csize_t, level, dataFormat: cint,
                 dst: ptr pointer, dstLen: ptr csize_t): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_uncompress(ctx: ZhCtx, src: pointer, len: csize_t, dataFormat: cint,
                   dst: ptr pointer, dstLen: ptr csize_t): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_compress_batch(ctx: ZhCtx, srcs: ptr pointer, lens: ptr csize_t, n: csize_t,
                       level, dataFormat: cint, dsts: ptr pointer, dstLens: ptr csize_t,
                       statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_uncompress_batch(ctx: ZhCtx, srcs: ptr pointer, lens: ptr csize_t, n: csize_t,
                         dataFormat: cint, dsts: ptr pointer, dstLens: ptr csize_t,
                         statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_crc32(ctx: ZhCtx, src: pointer, len: csize_t, res: ptr uint32): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_adler32(ctx: ZhCtx, src: pointer, len: csize_t, res: ptr uint32): cint {.importc, cdecl, dynlib: zhLib.}

var ctx {.threadvar.}: ZhCtx   # one context per thread: contexts are thread-compatible

proc engine(): ZhCtx =
  if ctx.isNil:
    let st = zh_create(-1, nil, ctx.addr)
    if st != 0: raise newException(ZippyError, $zh_strerror(st))
  ctx

proc take(p: pointer, len: csize_t, st: cint): string =
  ## status -> ZippyError with the reference's message; result -> GC-owned string
  if st != 0:
    if p != nil: zh_free(p)
    raise newException(ZippyError, $zh_strerror(st))
  result = newString(len.int)
  if len > 0: copyMem(result[0].addr, p, len.int)
  zh_free(p)

proc hipCompress*(src: pointer, len: int, level = DefaultCompression,
                  dataFormat = dfGzip): string {.raises: [ZippyError].} =
  var dst: pointer
  var dstLen: csize_t
  let st = zh_compress(engine(), src, len.csize_t, level.cint, ord(dataFormat).cint,
                       dst.addr, dstLen.addr)
  take(dst, dstLen, st)

proc hipUncompress*(src: pointer, len: int,
                    dataFormat = dfDetect): string {.raises: [ZippyError].} =
  var dst: pointer
  var dstLen: csize_t
  let st = zh_uncompress(engine(), src, len.csize_t, ord(dataFormat).cint,
                         dst.addr, dstLen.addr)
  take(dst, dstLen, st)

proc hipCompressBatch*(srcs: openArray[string], level = DefaultCompression,
                       dataFormat = dfGzip): seq[string] {.raises: [ZippyError].} =
  ## n independent compress() calls in one launch sequence (the shape the GPU wants)
  let n = srcs.len
  var
    ptrs = newSeq[pointer](n)
    lens = newSeq[csize_t](n)
    dsts = newSeq[pointer](n)
    dlens = newSeq[csize_t](n)
    sts = newSeq[int32](n)
  for i, s in srcs:
    ptrs[i] = if s.len > 0: s[0].unsafeAddr else: nil
    lens[i] = s.len.csize_t
  let rc = zh_compress_batch(engine(), ptrs[0].addr, lens[0].addr, n.csize_t, level.cint,
                             ord(dataFormat).cint, dsts[0].addr, dlens[0].addr, sts[0].addr)
  if rc != 0: raise newException(ZippyError, $zh_strerror(rc))
  for i in 0 ..< n: result.add take(dsts[i], dlens[i], sts[i].cint)

# ---- results into Nim strings the shim owns (zh_*_batch_into); contract mode for BestSpeed ----
proc zh_compress_bound(len: csize_t, dataFormat: cint): csize_t {.importc, cdecl, dynlib: zhLib.}
proc zh_compress_batch_into(ctx: ZhCtx, srcs: ptr pointer, lens: ptr csize_t, n: csize_t,
                            level, dataFormat: cint, dsts: ptr pointer, caps: ptr csize_t,
                            dstLens: ptr csize_t, statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_uncompress_batch_into(ctx: ZhCtx, srcs: ptr pointer, lens: ptr csize_t, n: csize_t,
                              dataFormat: cint, dsts: ptr pointer, caps: ptr csize_t,
                              dstLens: ptr csize_t, statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_set_l1_parse(ctx: ZhCtx, mode: cint) {.importc, cdecl, dynlib: zhLib.}

proc hipCompressBatchInto*(srcs: openArray[string], level = DefaultCompression,
                           dataFormat = dfGzip): seq[string] {.raises: [ZippyError].} =
  ## as hipCompressBatch, without the library's malloc + the copy out of it: the results land in
  ## strings this proc allocated (newString(bound), then setLen to what was written)
  let n = srcs.len
  result = newSeq[string](n)
  var
    ptrs = newSeq[pointer](n)
    lens = newSeq[csize_t](n)
    dsts = newSeq[pointer](n)
    caps = newSeq[csize_t](n)
    dlens = newSeq[csize_t](n)
    sts = newSeq[int32](n)
  for i, s in srcs:
    ptrs[i] = if s.len > 0: s[0].unsafeAddr else: nil
    lens[i] = s.len.csize_t
    caps[i] = zh_compress_bound(lens[i], ord(dataFormat).cint)
    result[i] = newString(caps[i].int)
    dsts[i] = result[i][0].addr
  let rc = zh_compress_batch_into(engine(), ptrs[0].addr, lens[0].addr, n.csize_t, level.cint,
                                  ord(dataFormat).cint, dsts[0].addr, caps[0].addr, dlens[0].addr, sts[0].addr)
  if rc != 0: raise newException(ZippyError, $zh_strerror(rc))
  for i in 0 ..< n:
    if sts[i] != 0: raise newException(ZippyError, $zh_strerror(sts[i].cint))
    result[i].setLen(dlens[i].int)

proc useParallelBestSpeedParse*(on = true) =
  ## BestSpeed only.  OFF (default): zippy's own parse, the streams are byte for byte zippy's.
  ## ON: a different token stream of about the same size (measured: 1-4 % smaller) that zippy's
  ## uncompress() decodes to the same bytes -- 2.4 x faster match finding on the device.
  zh_set_l1_parse(engine(), if on: 1 else: 0)

# ---- more than one GPU ----
proc zh_device_count(): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_compress_batch_multi(ctxs: ptr ZhCtx, nCtx: csize_t, srcs: ptr pointer, lens: ptr csize_t,
                             n: csize_t, level, dataFormat: cint, dsts: ptr pointer,
                             dstLens: ptr csize_t, statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_uncompress_batch_multi(ctxs: ptr ZhCtx, nCtx: csize_t, srcs: ptr pointer, lens: ptr csize_t,
                               n: csize_t, dataFormat: cint, dsts: ptr pointer, dstLens: ptr csize_t,
                               statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}

# ---- device-resident batches (one process a GPU: buffers and slots already in HBM, e.g. on their way between GPUs) ----
type ZhPlan = pointer
proc zh_plan_compress(ctx: ZhCtx, n: csize_t, srcOff, srcLen, dstOff, dstCap: ptr uint64, level, dataFormat: cint,
                      plan: ptr ZhPlan): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_plan_uncompress(ctx: ZhCtx, n: csize_t, srcOff, srcLen, dstOff, dstCap: ptr uint64, dataFormat: cint,
                        plan: ptr ZhPlan): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_plan_run(plan: ZhPlan, dSrc, dDst: pointer): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_plan_results(plan: ZhPlan, outLens: ptr uint64, statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_plan_pack(plan: ZhPlan, dSlots, dPacked: pointer, packedCap: uint64,
                  dOffsets: ptr uint64): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_plan_unpack(plan: ZhPlan, dPacked: pointer, dOffsets: ptr uint64,
                    dSlots: pointer): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_plan_destroy(plan: ZhPlan) {.importc, cdecl, dynlib: zhLib.}
proc zh_device_malloc(ctx: ZhCtx, bytes: csize_t, dOut: ptr pointer): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_device_free(ctx: ZhCtx, d: pointer) {.importc, cdecl, dynlib: zhLib.}
proc zh_device_upload(ctx: ZhCtx, dDst, src: pointer, bytes: csize_t): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_device_download(ctx: ZhCtx, dst, dSrc: pointer, bytes: csize_t): cint {.importc, cdecl, dynlib: zhLib.}

# ---- the archive layer (src/zippy/ziparchives.nim) ----
type
  ZhZipEntry {.bycopy.} = object
    path: cstring                       # not NUL-terminated: use pathLen
    pathLen: csize_t
    isDirectory: cint
    headerOffset, compressedSize, uncompressedSize: uint64
    crc32, unixMode: uint32

proc zh_zip_open(archive: pointer, len: csize_t, reader: ptr pointer): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_zip_close(reader: pointer) {.importc, cdecl, dynlib: zhLib.}
proc zh_zip_num_entries(reader: pointer): csize_t {.importc, cdecl, dynlib: zhLib.}
proc zh_zip_entry_at(reader: pointer, i: csize_t, e: ptr ZhZipEntry): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_zip_extract_batch(ctx: ZhCtx, reader: pointer, indices: ptr csize_t, n: csize_t,
                          dsts: ptr pointer, lens: ptr csize_t, statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_zip_create(ctx: ZhCtx, paths: ptr cstring, pathLens: ptr csize_t, contents: ptr pointer,
                   contentLens: ptr csize_t, n: csize_t, dosTime, dosDate: uint16,
                   archive: ptr pointer, archiveLen: ptr csize_t): cint {.importc, cdecl, dynlib: zhLib.}

proc hipCreateZipArchive*(entries: OrderedTable[string, string]): string {.raises: [ZippyError].} =
  ## createZipArchiveImpl (ziparchives.nim:455-623) with the per-entry codec work in one batch
  var paths: seq[cstring]; var pathLens, contentLens: seq[csize_t]; var contents: seq[pointer]
  for k, v in entries:                 # insertion order; the library lists them last to first
    paths.add k.cstring; pathLens.add k.len.csize_t
    contents.add (if v.len > 0: v[0].unsafeAddr else: nil); contentLens.add v.len.csize_t
  let (t, d) = msdos(getTime())        # ziparchives.nim:475-493, unchanged
  var p: pointer; var n: csize_t
  let st = zh_zip_create(engine(), paths[0].addr, pathLens[0].addr, contents[0].addr,
                         contentLens[0].addr, paths.len.csize_t, t, d, p.addr, n.addr)
  take(p, n, st)

# ---- writing tarballs (src/zippy/tarballs_v1.nim) ----
type
  ZhTarNewEntry {.bycopy.} = object
    path: cstring                       # not NUL-terminated: use pathLen
    pathLen: csize_t
    contents: pointer
    len: csize_t
    kind: char                          # '0' ekNormalFile, '5' ekDirectory
    mtime: int64                        # lastModified.toUnix

const ZH_TAR_PLAIN = -1.cint

proc zh_tar_create_batch(ctx: ZhCtx, entries: ptr ZhTarNewEntry, first: ptr csize_t, nTar: csize_t,
                         dataFormat, level: cint, dsts: ptr pointer, dstLens: ptr csize_t,
                         statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}

proc hipTarballImage*(entries: openArray[tuple[path, contents: string, kind: char, mtime: int64]],
                      gzip: bool): string {.raises: [ZippyError].} =
  ## writeTarball's `data` (tarballs_v1.nim:209-261), and with gzip its compress(data, DefaultCompression, dfGzip)
  ## (:269), in one call: headers, padding and trailer are written on the device
  var es = newSeq[ZhTarNewEntry](entries.len)
  for i, e in entries:                 # insertion order
    es[i] = ZhTarNewEntry(path: e.path.cstring, pathLen: e.path.len.csize_t,
                          contents: (if e.contents.len > 0: e.contents[0].unsafeAddr else: nil),
                          len: e.contents.len.csize_t, kind: e.kind, mtime: e.mtime)
  var first = [0.csize_t, es.len.csize_t]
  var p: pointer; var n: csize_t; var st: int32
  let rc = zh_tar_create_batch(engine(), (if es.len > 0: es[0].addr else: nil), first[0].addr, 1,
                               (if gzip: dfGzip.cint else: ZH_TAR_PLAIN), DefaultCompression.cint,
                               p.addr, n.addr, st.addr)
  take(p, n, if rc != 0: rc else: st.cint)

# ---- reading tarballs in batches (src/zippy/tarballs.nim extractAll) ----
type
  ZhTarEntry {.bycopy.} = object
    path: cstring                       # not NUL-terminated: use pathLen
    pathLen: csize_t
    linkname: cstring                   # symlinks (typeflag '2'); not NUL-terminated: use linknameLen
    linknameLen: csize_t
    typeflag: char                      # '0' or '\0' file, '5' directory, '2' symlink
    mode: uint32
    mtime: int64
    offset, size: uint64                # the entry's bytes inside zh_tar_data()
  HipTarEntry* = object
    path*, linkname*, contents*: string
    typeflag*: char
    mode*: uint32
    mtime*: int64

proc zh_tar_open_batch(ctx: ZhCtx, images: ptr pointer, lens: ptr csize_t, nTar: csize_t,
                       readers: ptr pointer, statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_tar_close(reader: pointer) {.importc, cdecl, dynlib: zhLib.}
proc zh_tar_num_entries(reader: pointer): csize_t {.importc, cdecl, dynlib: zhLib.}
proc zh_tar_entry_at(reader: pointer, i: csize_t, e: ptr ZhTarEntry): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_tar_data(reader: pointer, len: ptr csize_t): pointer {.importc, cdecl, dynlib: zhLib.}

proc hipOpenTarballs*(images: openArray[string]): seq[seq[HipTarEntry]] {.raises: [ZippyError].} =
  ## the loop body of extractAll (tarballs.nim:40-124) for many tarballs in one call: every .tar.gz gunzipped
  ## (trustSize) in one batch, every header walk on the device; raises on the first image that failed, as the
  ## reference would on that file.  The caller keeps createDir / writeFile / permissions / mtimes (:98-131).
  let n = images.len
  if n == 0: return
  var
    ptrs = newSeq[pointer](n)
    lens = newSeq[csize_t](n)
    readers = newSeq[pointer](n)
    sts = newSeq[int32](n)
  for i, s in images:
    ptrs[i] = if s.len > 0: s[0].unsafeAddr else: nil
    lens[i] = s.len.csize_t
  let rc = zh_tar_open_batch(engine(), ptrs[0].addr, lens[0].addr, n.csize_t, readers[0].addr, sts[0].addr)
  try:
    if rc != 0: raise newException(ZippyError, $zh_strerror(rc))
    for st in sts:
      if st != 0: raise newException(ZippyError, $zh_strerror(st.cint))
    result = newSeq[seq[HipTarEntry]](n)
    for t in 0 ..< n:
      var dataLen: csize_t
      let data = cast[ptr UncheckedArray[char]](zh_tar_data(readers[t], dataLen.addr))
      for i in 0 ..< zh_tar_num_entries(readers[t]).int:
        var e: ZhTarEntry
        discard zh_tar_entry_at(readers[t], i.csize_t, e.addr)
        var item = HipTarEntry(typeflag: e.typeflag, mode: e.mode, mtime: e.mtime)
        item.path = newString(e.pathLen.int)
        if e.pathLen > 0: copyMem(item.path[0].addr, e.path, e.pathLen.int)
        item.linkname = newString(e.linknameLen.int)
        if e.linknameLen > 0: copyMem(item.linkname[0].addr, e.linkname, e.linknameLen.int)
        item.contents = newString(e.size.int)
        if e.size > 0: copyMem(item.contents[0].addr, data[e.offset.int].addr, e.size.int)
        result[t].add item
  finally:
    for r in readers:
      if r != nil: zh_tar_close(r)

# ---- reading zip archives in batches (src/zippy/ziparchives.nim openZipArchive + extractAll) ----
# (ZhZipEntry, zh_zip_close, zh_zip_num_entries and zh_zip_entry_at are the archive layer's, above)
type
  HipZipEntry* = object
    path*, contents*: string
    isDirectory*: bool
    unixMode*: uint32

proc zh_zip_open_all_batch(ctx: ZhCtx, images: ptr pointer, lens: ptr csize_t, nZip: csize_t,
                           readers: ptr pointer, statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_zip_entry_data(reader: pointer, i: csize_t, data: ptr pointer, len: ptr csize_t,
                       status: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}

proc hipOpenZipArchives*(images: openArray[string]): seq[seq[HipZipEntry]] {.raises: [ZippyError].} =
  ## openZipArchive (ziparchives.nim:183-372) and the extraction loop of extractAll (:417-429) for many archives in
  ## one call: the directories walked, every entry decoded and its CRC-32 verified on the device; raises on the first
  ## archive whose status is not zero, as the reference would on that file.  The caller keeps createDir / writeFile /
  ## permissions / mtimes (:421-453).
  let n = images.len
  if n == 0: return
  var
    ptrs = newSeq[pointer](n)
    lens = newSeq[csize_t](n)
    readers = newSeq[pointer](n)
    sts = newSeq[int32](n)
  for i, s in images:
    ptrs[i] = if s.len > 0: s[0].unsafeAddr else: nil
    lens[i] = s.len.csize_t
  let rc = zh_zip_open_all_batch(engine(), ptrs[0].addr, lens[0].addr, n.csize_t, readers[0].addr, sts[0].addr)
  try:
    if rc != 0: raise newException(ZippyError, $zh_strerror(rc))
    for st in sts:
      if st != 0: raise newException(ZippyError, $zh_strerror(st.cint))
    result = newSeq[seq[HipZipEntry]](n)
    for t in 0 ..< n:
      for i in 0 ..< zh_zip_num_entries(readers[t]).int:
        var e: ZhZipEntry
        var data: pointer
        var len: csize_t
        var st: int32
        discard zh_zip_entry_at(readers[t], i.csize_t, e.addr)
        discard zh_zip_entry_data(readers[t], i.csize_t, data.addr, len.addr, st.addr)
        var item = HipZipEntry(isDirectory: e.isDirectory != 0, unixMode: e.unixMode)
        item.path = newString(e.pathLen.int)
        if e.pathLen > 0: copyMem(item.path[0].addr, e.path, e.pathLen.int)
        item.contents = newString(len.int)
        if len > 0: copyMem(item.contents[0].addr, data, len.int)
        result[t].add item
  finally:
    for r in readers:
      if r != nil: zh_zip_close(r)

# ---- writing zip archives (src/zippy/ziparchives_v1.nim) ----
import std/times

type
  ZhZipNewEntry {.bycopy.} = object
    path: cstring                       # not NUL-terminated: use pathLen
    pathLen: csize_t
    contents: pointer
    len: csize_t
    isDirectory: cint                   # ekDirectory: external attributes 0x10, else 0x20
    dosTime, dosDate: uint16            # toMsDos(lastModified)

proc zh_zip_write_batch(ctx: ZhCtx, entries: ptr ZhZipNewEntry, first: ptr csize_t, nZip: csize_t,
                        level: cint, dsts: ptr pointer, dstLens: ptr csize_t,
                        statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}

proc hipMsDos(t: Time): (uint16, uint16) =
  ## toMsDos (ziparchives_v1.nim:356-369), field for field: the reference's proc is private to its module
  let d = t.local()
  let years = max(0, d.year - 1980).uint16
  ((d.second div 2).uint16 or (d.minute.uint16 shl 5) or (d.hour.uint16 shl 11),
   d.monthday.uint16 or (ord(d.month).uint16 shl 5) or (years shl 9))

proc hipWriteZipArchive*[ZipArchive](archive: ZipArchive): string {.raises: [ZippyError].} =
  ## writeZipArchive's `data` (ziparchives_v1.nim:371-479) in one call: every entry's compress(contents,
  ## DefaultCompression, dfDeflate) and crc32, and every header, written on the device.  Generic in the archive type
  ## (ziparchives_v1.ZipArchive), so that this module does not import the module that calls it.
  var paths: seq[string]               # the keys, kept alive for the call
  var es: seq[ZhZipNewEntry]
  for path, e in archive.contents.mpairs:   # insertion order; `e` is the table's own entry
    let (t, d) = hipMsDos(e.lastModified)
    paths.add path
    es.add ZhZipNewEntry(pathLen: path.len.csize_t,
                         contents: (if e.contents.len > 0: e.contents[0].addr else: nil),
                         len: e.contents.len.csize_t, isDirectory: cint(ord(e.kind) == 1),  # ekFile, ekDirectory
                         dosTime: t, dosDate: d)
  for i in 0 ..< es.len:
    es[i].path = paths[i].cstring
  var first = [0.csize_t, es.len.csize_t]
  var p: pointer; var n: csize_t; var st: int32
  let rc = zh_zip_write_batch(engine(), (if es.len > 0: es[0].addr else: nil), first[0].addr, 1,
                              DefaultCompression.cint, p.addr, n.addr, st.addr)
  take(p, n, if rc != 0: rc else: st.cint)

import std/os

# ---- ZipArchive.open (src/zippy/ziparchives_v1.nim:105-349 openStreamImpl) ----
type
  HipZipV1Entry* = object
    path*, contents*: string            # the table's key (toUnixPath of the name), the verified contents
    isDirectory*, inDirectory*: bool    # external attributes & 0x10; a central record named the entry
    unixMode*: uint32                   # external attributes shr 16 (0 without a central record)
    dosTime*, dosDate*: uint16          # the local record's words (:128-129)

proc zh_zip_read_batch(ctx: ZhCtx, images: ptr pointer, lens: ptr csize_t, nZip: csize_t,
                       readers: ptr pointer, statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_zip_entry_v1(reader: pointer, i: csize_t, dosTime, dosDate: ptr uint16,
                     inDirectory: ptr cint): cint {.importc, cdecl, dynlib: zhLib.}

proc hipReadZipArchives*(images: openArray[string]): seq[seq[HipZipV1Entry]] {.raises: [ZippyError].} =
  ## openStreamImpl (ziparchives_v1.nim:105-329) for many images in one call: every image walked from byte 0, every
  ## entry decoded, its CRC-32 and its length verified on the device; an image's entries are its table's keys in
  ## insertion order.  Raises on the first image whose status is not zero, as the reference would on that stream
  ## (without the half-filled table the reference leaves behind its exception).
  let n = images.len
  if n == 0: return
  var
    ptrs = newSeq[pointer](n)
    lens = newSeq[csize_t](n)
    readers = newSeq[pointer](n)
    sts = newSeq[int32](n)
  for i, s in images:
    ptrs[i] = if s.len > 0: s[0].unsafeAddr else: nil
    lens[i] = s.len.csize_t
  let rc = zh_zip_read_batch(engine(), ptrs[0].addr, lens[0].addr, n.csize_t, readers[0].addr, sts[0].addr)
  try:
    if rc != 0: raise newException(ZippyError, $zh_strerror(rc))
    for st in sts:
      if st != 0: raise newException(ZippyError, $zh_strerror(st.cint))
    result = newSeq[seq[HipZipV1Entry]](n)
    for t in 0 ..< n:
      for i in 0 ..< zh_zip_num_entries(readers[t]).int:
        var e: ZhZipEntry
        var data: pointer
        var len: csize_t
        var st: int32
        var inDir: cint
        var item: HipZipV1Entry
        discard zh_zip_entry_at(readers[t], i.csize_t, e.addr)
        discard zh_zip_entry_data(readers[t], i.csize_t, data.addr, len.addr, st.addr)
        discard zh_zip_entry_v1(readers[t], i.csize_t, item.dosTime.addr, item.dosDate.addr, inDir.addr)
        item.isDirectory = e.isDirectory != 0
        item.inDirectory = inDir != 0
        item.unixMode = e.unixMode
        item.path = newString(e.pathLen.int)
        if e.pathLen > 0: copyMem(item.path[0].addr, e.path, e.pathLen.int)
        item.contents = newString(len.int)
        if len > 0: copyMem(item.contents[0].addr, data, len.int)
        result[t].add item
  finally:
    for r in readers:
      if r != nil: zh_zip_close(r)

proc hipDosTime*(dosTime, dosDate: uint16): Time =
  ## ziparchives_v1.nim:161-179, field for field: the caller's zone; a Defect for day or month 0, as there
  let
    seconds = (dosTime and 0b0000000000011111).int * 2
    minutes = ((dosTime shr 5) and 0b0000000000111111).int
    hours = ((dosTime shr 11) and 0b0000000000011111).int
    days = (dosDate and 0b0000000000011111).int
    months = ((dosDate shr 5) and 0b0000000000001111).int
    years = ((dosDate shr 9) and 0b0000000001111111).int
  if seconds <= 59 and minutes <= 59 and hours <= 23:
    result = initDateTime(days.MonthdayRange, months.Month, years + 1980, hours.HourRange, minutes.MinuteRange,
                          seconds.SecondRange, local()).toTime()

proc hipPermissions*(unixMode: uint32): set[FilePermission] =
  ## extractPermissions (ziparchives_v1.nim:84-103) of externalFileAttr shr 16
  if defined(windows) or unixMode == 0:
    result = {fpUserRead, fpUserWrite, fpGroupRead, fpGroupWrite, fpOthersRead}
  else:
    if (unixMode and 0o00400) != 0: result.incl fpUserRead
    if (unixMode and 0o00200) != 0: result.incl fpUserWrite
    if (unixMode and 0o00100) != 0: result.incl fpUserExec
    if (unixMode and 0o00040) != 0: result.incl fpGroupRead
    if (unixMode and 0o00020) != 0: result.incl fpGroupWrite
    if (unixMode and 0o00010) != 0: result.incl fpGroupExec
    if (unixMode and 0o00004) != 0: result.incl fpOthersRead
    if (unixMode and 0o00002) != 0: result.incl fpOthersWrite
    if (unixMode and 0o00001) != 0: result.incl fpOthersExec

# ---- createZipArchive for many tables per call (src/zippy/ziparchives.nim:455-634) ----
proc zh_zip_create_batch(ctx: ZhCtx, entries: ptr ZhZipNewEntry, first: ptr csize_t, nZip: csize_t,
                         level: cint, dsts: ptr pointer, dstLens: ptr csize_t,
                         statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}

proc createZipArchives*(tables: seq[OrderedTable[string, string]]): seq[string] {.raises: [ZippyError].} =
  ## createZipArchive(entries) (ziparchives.nim:625-634) of every table in ONE call: all entries' compress(contents,
  ## BestSpeed, dfDeflate) and crc32 in one plan, every record of every archive written on the device.  One
  ## msdos(getTime()) stamps all entries, as the reference stamps those of one call (:475-493).  Raises on the first
  ## archive that failed.
  if tables.len == 0: return
  let (t, d) = msdos(getTime())
  var es: seq[ZhZipNewEntry]
  var first = @[0.csize_t]
  for table in tables:
    for k, v in table:                 # insertion order; the library lists them last to first
      es.add ZhZipNewEntry(path: k.cstring, pathLen: k.len.csize_t,
                           contents: (if v.len > 0: v[0].unsafeAddr else: nil), len: v.len.csize_t,
                           isDirectory: 0, dosTime: t, dosDate: d)   # isDirectory is not read
    first.add es.len.csize_t
  var ps = newSeq[pointer](tables.len); var ns = newSeq[csize_t](tables.len); var sts = newSeq[int32](tables.len)
  let rc = zh_zip_create_batch(engine(), (if es.len > 0: es[0].addr else: nil), first[0].addr, tables.len.csize_t,
                               BestSpeed.cint, ps[0].addr, ns[0].addr, sts[0].addr)
  var firstBad = rc
  for i in 0 ..< tables.len:           # copy what came back, free everything, then raise
    if firstBad == 0 and sts[i] != 0: firstBad = sts[i].cint
  for i in 0 ..< tables.len:
    if firstBad != 0:
      if ps[i] != nil: zh_free(ps[i])
    else:
      result.add take(ps[i], ns[i], 0)
  if firstBad != 0:
    raise newException(ZippyError, $zh_strerror(firstBad))

# ---- Tarball.open (src/zippy/tarballs_v1.nim:66-157 openStreamImpl) ----
type
  HipTarV1Entry* = object
    path*, contents*: string            # the table's key ((prefix / name).toUnixPath()), the contents
    kind*: char                         # '0' ekNormalFile, '5' ekDirectory (nothing else set, as :150-154)
    mode*: uint32                       # parseOctInt of the mode field's six bytes (a file's)
    mtime*: int64                       # parseOctInt of the mtime field (a file's)

proc zh_tar_read_batch(ctx: ZhCtx, images: ptr pointer, lens: ptr csize_t, formats: ptr int32, nTar: csize_t,
                       readers: ptr pointer, statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}

proc hipReadTarballs*(images: openArray[string],
                      formats: openArray[int32] = []): seq[seq[HipTarV1Entry]] {.raises: [ZippyError].} =
  ## openStreamImpl (tarballs_v1.nim:66-157) for many images in one call: every gzip image through one
  ## uncompress(data, dfGzip) batch, the header loop of :99-157 for all images at once on the device; an image's
  ## entries are its table's keys in the table's order.  formats: ord(tarballFormat) an image (tfDetect, tfUncompressed,
  ## tfGzip = 0, 1, 2); none: all tfDetect.  Raises on the first image whose status is not zero, as the reference
  ## would on that stream (without the half-filled table the reference leaves behind its exception).
  let n = images.len
  if n == 0: return
  if formats.len != 0 and formats.len != n:
    raise newException(ZippyError, "hipReadTarballs: one format an image")
  var
    ptrs = newSeq[pointer](n)
    lens = newSeq[csize_t](n)
    fmts = @formats
    readers = newSeq[pointer](n)
    sts = newSeq[int32](n)
  for i, s in images:
    ptrs[i] = if s.len > 0: s[0].unsafeAddr else: nil
    lens[i] = s.len.csize_t
  let rc = zh_tar_read_batch(engine(), ptrs[0].addr, lens[0].addr, (if fmts.len > 0: fmts[0].addr else: nil),
                             n.csize_t, readers[0].addr, sts[0].addr)
  try:
    if rc != 0: raise newException(ZippyError, $zh_strerror(rc))
    for st in sts:
      if st != 0: raise newException(ZippyError, $zh_strerror(st.cint))
    result = newSeq[seq[HipTarV1Entry]](n)
    for t in 0 ..< n:
      var dataLen: csize_t
      let data = cast[ptr UncheckedArray[char]](zh_tar_data(readers[t], dataLen.addr))
      for i in 0 ..< zh_tar_num_entries(readers[t]).int:
        var e: ZhTarEntry
        discard zh_tar_entry_at(readers[t], i.csize_t, e.addr)
        var item = HipTarV1Entry(kind: e.typeflag, mode: e.mode, mtime: e.mtime)
        item.path = newString(e.pathLen.int)
        if e.pathLen > 0: copyMem(item.path[0].addr, e.path, e.pathLen.int)
        item.contents = newString(e.size.int)
        if e.size > 0: copyMem(item.contents[0].addr, data[e.offset.int].addr, e.size.int)
        result[t].add item
  finally:
    for r in readers:
      if r != nil: zh_tar_close(r)

# ---- random access into block-indexed streams (no counterpart in the reference) ----
type
  ZhBlockEntry* {.bycopy.} = object
    bitOff*: uint64                     # the block's first bit, counted from the compressed buffer's first byte
    outOff*: uint64                     # its first byte in the uncompressed data; the closing entry: the length

proc zh_compress_blocks(ctx: ZhCtx, src: pointer, len: csize_t, level, dataFormat: cint, blockBytes: csize_t,
                        dst: ptr pointer, dstLen: ptr csize_t, index: ptr ptr ZhBlockEntry,
                        nEntries: ptr csize_t): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_uncompress_ranges(ctx: ZhCtx, srcs: ptr pointer, lens: ptr csize_t, nStreams: csize_t,
                          index: ptr ZhBlockEntry, first: ptr csize_t, nRanges: csize_t,
                          rangeStream, rangeOff, rangeLen: ptr uint64, dsts: ptr pointer, dstLens: ptr csize_t,
                          statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_plan_uncompress_ranges(ctx: ZhCtx, nStreams: csize_t, srcOff, srcLen: ptr uint64,
                               index: ptr ZhBlockEntry, first: ptr csize_t, nRanges: csize_t,
                               rangeStream, rangeOff, rangeLen, dstOff, dstCap: ptr uint64,
                               plan: ptr ZhPlan): cint {.importc, cdecl, dynlib: zhLib.}

proc hipCompressBlocks*(src: string, blockBytes = 32768, level = BestSpeed,
                        dataFormat = dfGzip): (string, seq[ZhBlockEntry]) {.raises: [ZippyError].} =
  ## compress() with deflate blocks of blockBytes (a multiple of 32768, up to 4 MiB) that no match crosses, and the
  ## index of their starts: still a stream uncompress() reads, and one hipReadRanges reads bytes out of
  var dst: pointer; var dstLen, n: csize_t; var idx: ptr ZhBlockEntry
  let st = zh_compress_blocks(engine(), (if src.len > 0: src[0].unsafeAddr else: nil), src.len.csize_t, level.cint,
                              ord(dataFormat).cint, blockBytes.csize_t, dst.addr, dstLen.addr, idx.addr, n.addr)
  if st == 0:
    result[1] = newSeq[ZhBlockEntry](n.int)
    copyMem(result[1][0].addr, idx, n.int * sizeof(ZhBlockEntry))
    zh_free(idx)
  result[0] = take(dst, dstLen, st)

proc hipReadRanges*(streams: openArray[string], indexes: openArray[seq[ZhBlockEntry]],
                    ranges: openArray[tuple[stream, off, len: uint64]]): seq[string] {.raises: [ZippyError].} =
  ## bytes [off, off + len) of the uncompressed data of streams[stream], for every range, in one call: only the
  ## blocks a range touches are uploaded and decoded.  Ranges read like pread (clipped at the end, empty behind it).
  ## Raises on the first range that could not be read (a damaged block, an index that does not fit its stream).
  let n = ranges.len
  if n == 0: return
  var
    ptrs = newSeq[pointer](max(1, streams.len))
    lens = newSeq[csize_t](max(1, streams.len))
    flat: seq[ZhBlockEntry]
    first = @[0.csize_t]
    rs = newSeq[uint64](n); ro = newSeq[uint64](n); rl = newSeq[uint64](n)
    dsts = newSeq[pointer](n); dlens = newSeq[csize_t](n); sts = newSeq[int32](n)
  for i, s in streams:
    ptrs[i] = if s.len > 0: s[0].unsafeAddr else: nil
    lens[i] = s.len.csize_t
    flat.add indexes[i]
    first.add flat.len.csize_t
  for i, r in ranges: (rs[i], ro[i], rl[i]) = (r.stream, r.off, r.len)
  let rc = zh_uncompress_ranges(engine(), ptrs[0].addr, lens[0].addr, streams.len.csize_t,
                                (if flat.len > 0: flat[0].addr else: nil), first[0].addr, n.csize_t,
                                rs[0].addr, ro[0].addr, rl[0].addr, dsts[0].addr, dlens[0].addr, sts[0].addr)
  var firstBad = rc
  for i in 0 ..< n:                    # copy what came back, free everything, then raise
    if firstBad == 0 and sts[i] != 0: firstBad = sts[i].cint
  for i in 0 ..< n:
    if firstBad != 0:
      if dsts[i] != nil: zh_free(dsts[i])
    else:
      result.add take(dsts[i], dlens[i], 0)
  if firstBad != 0:
    raise newException(ZippyError, $zh_strerror(firstBad))

# ---- BGZF: the blocked gzip of bgzip / htslib (no counterpart in the reference) ----
type
  ZhBgzfEntry* {.bycopy.} = object
    coff*: uint64                       # the member's first byte in the file; the closing entry: the file's end
    uoff*: uint64                       # its first byte in the uncompressed data; the closing entry: the total

proc zh_bgzf_write_batch(ctx: ZhCtx, srcs: ptr pointer, lens: ptr csize_t, n: csize_t, level: cint,
                         blockBytes: csize_t, dsts: ptr pointer, dstLens: ptr csize_t,
                         statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_bgzf_read_batch(ctx: ZhCtx, images: ptr pointer, lens: ptr csize_t, n: csize_t, dsts: ptr pointer,
                        dstLens: ptr csize_t, statuses: ptr int32,
                        hasEof: ptr uint8): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_bgzf_index_batch(ctx: ZhCtx, images: ptr pointer, lens: ptr csize_t, n: csize_t,
                         index: ptr ptr ZhBgzfEntry, first: ptr csize_t, statuses: ptr int32,
                         hasEof: ptr uint8): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_bgzf_read_ranges(ctx: ZhCtx, images: ptr pointer, lens: ptr csize_t, nImages: csize_t,
                         index: ptr ZhBgzfEntry, first: ptr csize_t, nRanges: csize_t,
                         rangeImage, rangeOff, rangeLen: ptr uint64, dsts: ptr pointer, dstLens: ptr csize_t,
                         statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}

proc compressBgzf*(src: string, level = DefaultCompression, blockBytes = 0): string {.raises: [ZippyError].} =
  ## src as a BGZF file: gzip members of blockBytes (0: 65280) uncompressed bytes each and the EOF marker;
  ## uncompress() of any gunzip reads it, and its index is in the file (hipBgzfIndex)
  var p = if src.len > 0: src[0].unsafeAddr.pointer else: nil
  var len = src.len.csize_t
  var dst: pointer; var dstLen: csize_t; var st: int32
  let rc = zh_bgzf_write_batch(engine(), p.addr, len.addr, 1, level.cint, blockBytes.csize_t, dst.addr, dstLen.addr,
                               st.addr)
  take(dst, dstLen, if rc != 0: rc else: st.cint)

proc uncompressBgzf*(image: string): string {.raises: [ZippyError].} =
  ## the uncompressed data of a BGZF file, every member verified by its CRC-32 and ISIZE
  var p = if image.len > 0: image[0].unsafeAddr.pointer else: nil
  var len = image.len.csize_t
  var dst: pointer; var dstLen: csize_t; var st: int32
  let rc = zh_bgzf_read_batch(engine(), p.addr, len.addr, 1, dst.addr, dstLen.addr, st.addr, nil)
  take(dst, dstLen, if rc != 0: rc else: st.cint)

proc hipBgzfIndex*(image: string): seq[ZhBgzfEntry] {.raises: [ZippyError].} =
  ## the members of a BGZF file from its headers and trailers alone, closed by (the file's end, the total)
  var p = if image.len > 0: image[0].unsafeAddr.pointer else: nil
  var len = image.len.csize_t
  var idx: ptr ZhBgzfEntry; var first: array[2, csize_t]; var st: int32; var eof: uint8
  let rc = zh_bgzf_index_batch(engine(), p.addr, len.addr, 1, idx.addr, first[0].addr, st.addr, eof.addr)
  if rc == 0 and st == 0:
    result = newSeq[ZhBgzfEntry](first[1].int)
    copyMem(result[0].addr, idx, first[1].int * sizeof(ZhBgzfEntry))
  if idx != nil: zh_free(idx)
  if rc != 0 or st != 0:
    raise newException(ZippyError, $zh_strerror(if rc != 0: rc else: st.cint))

proc hipBgzfReadRange*(image: string, index: seq[ZhBgzfEntry], off, len: uint64): string {.raises: [ZippyError].} =
  ## bytes [off, off + len) of the uncompressed data: only the members the range touches are uploaded and decoded,
  ## each verified by its checksum.  Reads like pread (clipped at the end, empty behind it).
  var p = if image.len > 0: image[0].unsafeAddr.pointer else: nil
  var ilen = image.len.csize_t
  var first = [0.csize_t, index.len.csize_t]
  var ri = 0'u64; var ro = off; var rl = len
  var dst: pointer; var dstLen: csize_t; var st: int32
  let rc = zh_bgzf_read_ranges(engine(), p.addr, ilen.addr, 1, (if index.len > 0: index[0].unsafeAddr else: nil),
                               first[0].addr, 1, ri.addr, ro.addr, rl.addr, dst.addr, dstLen.addr, st.addr)
  take(dst, dstLen, if rc != 0: rc else: st.cint)

# ---- seek indexes for foreign deflate streams (no counterpart in the reference) ----
proc zh_seek_index_batch(ctx: ZhCtx, srcs: ptr pointer, lens: ptr csize_t, n: csize_t, dataFormat: cint, span: uint64,
                         indexes: ptr pointer, indexLens: ptr csize_t, dsts: ptr pointer, dstLens: ptr csize_t,
                         statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_seek_read_ranges(ctx: ZhCtx, srcs: ptr pointer, lens: ptr csize_t, nStreams: csize_t, indexes: ptr pointer,
                         indexLens: ptr csize_t, nRanges: csize_t, rangeStream, rangeOff, rangeLen: ptr uint64,
                         dsts: ptr pointer, dstLens: ptr csize_t,
                         statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}

proc hipSeekIndex*(src: string, dataFormat = dfDetect, span = 0'u64): string {.raises: [ZippyError].} =
  ## the seek index of a zlib / gzip / raw deflate stream of any writer: a blob that may be stored (the layout is
  ## include/zippy_hip.h's); span: uncompressed bytes between points (0: 1 MiB, else at least 32768)
  var p = if src.len > 0: src[0].unsafeAddr.pointer else: nil
  var len = src.len.csize_t
  var idx: pointer; var idxLen: csize_t; var st: int32
  let rc = zh_seek_index_batch(engine(), p.addr, len.addr, 1, dataFormat.cint, span, idx.addr, idxLen.addr, nil, nil,
                               st.addr)
  take(idx, idxLen, if rc != 0: rc else: st.cint)

proc hipSeekReadRange*(src, index: string, off, len: uint64): string {.raises: [ZippyError].} =
  ## bytes [off, off + len) of the uncompressed data: only the intervals the range touches and their windows are
  ## uploaded and decoded, each verified by its CRC-32.  Reads like pread (clipped at the end, empty behind it).
  var p = if src.len > 0: src[0].unsafeAddr.pointer else: nil
  var slen = src.len.csize_t
  var ip = if index.len > 0: index[0].unsafeAddr.pointer else: nil
  var ilen = index.len.csize_t
  var ri = 0'u64; var ro = off; var rl = len
  var dst: pointer; var dstLen: csize_t; var st: int32
  let rc = zh_seek_read_ranges(engine(), p.addr, slen.addr, 1, ip.addr, ilen.addr, 1, ri.addr, ro.addr, rl.addr,
                               dst.addr, dstLen.addr, st.addr)
  take(dst, dstLen, if rc != 0: rc else: st.cint)

# ---- resumable uncompress: a stream decoded as its bytes arrive (no counterpart in the reference) ----
const ZhResumeDone* = 0'i32; const ZhResumeNeedInput* = 1'i32; const ZhResumeNeedOutput* = 2'i32
proc zh_uncompress_resume_batch(ctx: ZhCtx, srcs: ptr pointer, lens: ptr csize_t, n: csize_t, dataFormat: cint,
                                states: ptr pointer, stateLens: ptr csize_t, maxOut: ptr uint64, last: ptr uint8,
                                dsts: ptr pointer, dstLens: ptr csize_t, consumed: ptr csize_t, newStates: ptr pointer,
                                newStateLens: ptr csize_t, why: ptr int32,
                                statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}

proc hipUncompressResume*(tail: string, state: var string, consumed: var int, why: var int32, maxOut = 1'u64 shl 20,
                          last = false, dataFormat = dfDetect): string {.raises: [ZippyError].} =
  ## one step of one stream: `tail` is what the step before left unconsumed followed by what arrived since, `state` the
  ## state that step returned ("" for a new stream; it is replaced).  Returns the bytes of the deflate blocks that became
  ## whole; why: ZhResumeDone (trailer verified), ZhResumeNeedInput, ZhResumeNeedOutput (a block larger than maxOut).
  var p = if tail.len > 0: tail[0].unsafeAddr.pointer else: nil
  var len = tail.len.csize_t
  var sp = if state.len > 0: state[0].unsafeAddr.pointer else: nil
  var slen = state.len.csize_t
  var mo = maxOut
  var lf = if last: 1'u8 else: 0'u8
  var dst, ns: pointer; var dstLen, used, nsLen: csize_t; var st: int32
  let rc = zh_uncompress_resume_batch(engine(), p.addr, len.addr, 1, dataFormat.cint, sp.addr, slen.addr, mo.addr,
                                      lf.addr, dst.addr, dstLen.addr, used.addr, ns.addr, nsLen.addr, why.addr, st.addr)
  var next = newString(nsLen.int)
  if ns != nil:
    if nsLen > 0: copyMem(next[0].addr, ns, nsLen.int)
    zh_free(ns)
  state = next
  consumed = used.int
  take(dst, dstLen, if rc != 0: rc else: st.cint)

# ---- streaming compress: a stream fed piece by piece, flushed, finished (no counterpart in the reference) ----
const ZhFlushBlock* = 0'u8; const ZhFlushSync* = 1'u8; const ZhFlushFinish* = 2'u8
proc zh_compress_stream_batch(ctx: ZhCtx, srcs: ptr pointer, lens: ptr csize_t, n: csize_t, level, dataFormat: cint,
                              blockBytes: csize_t, states: ptr pointer, stateLens: ptr csize_t, flush: ptr uint8,
                              dsts: ptr pointer, dstLens: ptr csize_t, newStates: ptr pointer,
                              newStateLens: ptr csize_t, statuses: ptr int32): cint {.importc, cdecl, dynlib: zhLib.}

proc hipCompressStream*(piece: string, state: var string, flush = ZhFlushSync, level = DefaultCompression,
                        dataFormat = dfGzip, blockBytes = 0): string {.raises: [ZippyError].} =
  ## one step of one stream: `piece` is its next bytes, `state` the state the step before returned ("" for a new stream,
  ## which takes level, dataFormat and blockBytes -- 0: 4 MiB -- from this call; a step that succeeds replaces it, with ""
  ## behind ZhFlushFinish, and a step that raises leaves it as it was).  Returns the whole bytes the stream has made since the step before.
  var p = if piece.len > 0: piece[0].unsafeAddr.pointer else: nil
  var len = piece.len.csize_t
  var sp = if state.len > 0: state[0].unsafeAddr.pointer else: nil
  var slen = state.len.csize_t
  var fl = flush
  var dst, ns: pointer; var dstLen, nsLen: csize_t; var st: int32
  let rc = zh_compress_stream_batch(engine(), p.addr, len.addr, 1, level.cint, dataFormat.cint, blockBytes.csize_t,
                                    sp.addr, slen.addr, fl.addr, dst.addr, dstLen.addr, ns.addr, nsLen.addr, st.addr)
  if rc == 0 and st == 0:  # (a failed step leaves the state as it was: the caller may try again with it)
    var next = newString(nsLen.int)
    if ns != nil and nsLen > 0: copyMem(next[0].addr, ns, nsLen.int)
    state = next
  if ns != nil: zh_free(ns)
  take(dst, dstLen, if rc != 0: rc else: st.cint)

# ---- any gzip file: several members, FEXTRA / FNAME / FCOMMENT / FHCRC (no counterpart in the reference) ----
type
  ZhGzipMember* {.bycopy.} = object
    coff*, cdataOff*, cdataLen*: uint64  # in the file: first header byte, first deflate byte, deflate bytes
    uoff*, ulen*: uint64                 # in the uncompressed data
    crc*, isize*, mtime*: uint32         # trailer, header
    flg*, xfl*, os*, pad*: uint8
    extraOff*, extraLen*, nameOff*, nameLen*, commentOff*, commentLen*: uint32  # from coff; 0 / 0 when absent

proc zh_gzip_read_batch(ctx: ZhCtx, images: ptr pointer, lens: ptr csize_t, n: csize_t, dsts: ptr pointer,
                        dstLens: ptr csize_t, statuses: ptr int32, members: ptr ptr ZhGzipMember,
                        first: ptr csize_t): cint {.importc, cdecl, dynlib: zhLib.}
proc zh_debug_gzip_stats(ctx: ZhCtx, candidates, speculativeBytes,
                         frontierRounds: ptr uint64): cint {.importc, cdecl, dynlib: zhLib.}

proc uncompressGzipFile*(image: string): string {.raises: [ZippyError].} =
  ## the uncompressed data of a gzip file of any shape: its members' data back to back (cat a.gz b.gz, appended logs,
  ## pigz -i, .warc.gz; FEXTRA, FNAME, FCOMMENT, FHCRC), every member verified by its CRC-32 and ISIZE
  var p = if image.len > 0: image[0].unsafeAddr.pointer else: nil
  var len = image.len.csize_t
  var dst: pointer; var dstLen: csize_t; var st: int32
  let rc = zh_gzip_read_batch(engine(), p.addr, len.addr, 1, dst.addr, dstLen.addr, st.addr, nil, nil)
  take(dst, dstLen, if rc != 0: rc else: st.cint)

proc hipGzipMembers*(image: string): seq[ZhGzipMember] {.raises: [ZippyError].} =
  ## the members of a gzip file, each decoded and verified on the device; no data comes down
  var p = if image.len > 0: image[0].unsafeAddr.pointer else: nil
  var len = image.len.csize_t
  var mem: ptr ZhGzipMember; var first: array[2, csize_t]; var st: int32
  let rc = zh_gzip_read_batch(engine(), p.addr, len.addr, 1, nil, nil, st.addr, mem.addr, first[0].addr)
  if rc == 0 and st == 0 and first[1] > 0:
    result = newSeq[ZhGzipMember](first[1].int)
    copyMem(result[0].addr, mem, first[1].int * sizeof(ZhGzipMember))
  if mem != nil: zh_free(mem)
  if rc != 0 or st != 0:
    raise newException(ZippyError, $zh_strerror(if rc != 0: rc else: st.cint))
