// What zh_zip.hip (zh_zip_open, one archive, host) and the batch readers (zh_zip_open_batch.hip: zh_zip_open_all_batch;
// zh_zip_read_batch.hip: zh_zip_read_batch; many archives, device) share: where an image's central directory is, the CP437 conversion, and the readers the batch call builds
// from its kernels' records.  Host code only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/zippy_hip.h"

#define ZH_ZIP_INTERNAL __attribute__((visibility("hidden")))

// openZipArchive up to its record loop (ziparchives.nim:162-268): the end records, the disk / record number checks,
// the sanity bounds, and the first central header found by counting signatures backwards.
struct ZhZipDirectory {
  int64_t num_records, cd_size, cd_start;
  int64_t socd;  // position of the first central header; socd_offset = socd - cd_start
};
ZH_ZIP_INTERNAL int zh_zip_locate(const void* archive, size_t len, ZhZipDirectory* out);

// a name without the language-encoding flag that is not valid UTF-8: code page 437 -> UTF-8 (ziparchives.nim:108-160)
ZH_ZIP_INTERNAL std::string zh_zip_from_cp437(const char* name, size_t len);

// The readers of the batch call: an empty reader over the borrowed image, its records in directory order (the path
// as it is reported, after any conversion), then the results of the extraction: entry i's bytes are
// block[off[i], + len[i]) -- or, for an entry that was redone on its own, redone[i] (malloc'ed, the reader's from
// here on) -- with status[i]; `block` (malloc'ed, may be NULL) becomes the reader's.
ZH_ZIP_INTERNAL zh_zip_reader* zh_zip_reader_new(const void* image, size_t len);
ZH_ZIP_INTERNAL void zh_zip_reader_add(zh_zip_reader* r, std::string path, bool directory, int64_t header_offset,
                                       uint32_t crc, int64_t compressed_size, int64_t uncompressed_size,
                                       uint32_t unix_mode);
ZH_ZIP_INTERNAL void zh_zip_reader_set_data(zh_zip_reader* r, void* block, size_t block_len, const uint64_t* off,
                                            const uint64_t* len, const int32_t* status, void* const* redone);
// A reader of zh_zip_read_batch (ziparchives_v1.nim's table): per entry the DOS time and date words of its local record
// and whether a central record named it.  zh_zip_extract_batch refuses such a reader (its entries are all extracted).
ZH_ZIP_INTERNAL void zh_zip_reader_set_v1(zh_zip_reader* r, const uint16_t* dos_time, const uint16_t* dos_date,
                                          const uint8_t* in_directory);
