// Stand-alone driver for the host side of zh_zip_read_batch under -fsanitize=address,undefined (built by
// tests/test_zip_read_sanitize.py from zippy_amd/csrc against the emulator runtime of tests/hipemu): opens the images
// of a directory (NAME.zip, with expected.txt: "NAME.zip STATUS" a line; -1: a status of the decoder's) each by
// itself and all in one call, holds the statuses against the expected ones, and reads every field and byte of every
// reader.
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "../include/zippy_hip.h"

static int check_reader(zh_ctx* ctx, zh_zip_reader* r, unsigned long* sum) {
  const size_t n = zh_zip_num_entries(r);
  for (size_t i = 0; i < n; i++) {
    zh_zip_entry e;
    const void* data;
    size_t len, found;
    int32_t st;
    uint16_t t, d;
    int in_dir;
    if (zh_zip_entry_at(r, i, &e) || zh_zip_entry_data(r, i, &data, &len, &st) || st != ZH_OK ||
        zh_zip_entry_v1(r, i, &t, &d, &in_dir) || zh_zip_find(r, e.path, e.path_len, &found) || found != i ||
        len != e.uncompressed_size)
      return 1;
    for (size_t k = 0; k < e.path_len; k++) *sum += (unsigned char)e.path[k];
    for (size_t k = 0; k < len; k++) *sum += ((const unsigned char*)data)[k];
    *sum += t + d + in_dir;
  }
  uint16_t t, d;
  int in_dir;
  size_t idx = 0;
  void* dst = nullptr;
  size_t dlen = 0;
  int32_t dst_st = 0;
  if (zh_zip_entry_v1(r, n, &t, &d, &in_dir) != ZH_ERR_ARGUMENT) return 1;
  if (zh_zip_extract_batch(ctx, r, &idx, n ? 1 : 0, &dst, &dlen, &dst_st) != ZH_ERR_ARGUMENT) return 1;
  size_t blen;
  const unsigned char* block = (const unsigned char*)zh_zip_data(r, &blen);
  if (block) *sum += block[0] + block[blen - 1];
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  std::ifstream list(dir + "/expected.txt");
  std::vector<std::string> images;
  std::vector<int> want;
  std::string name;
  int status;
  while (list >> name >> status) {
    std::ifstream f(dir + "/" + name, std::ios::binary);
    images.emplace_back(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    want.push_back(status);
  }
  const size_t n = images.size();
  if (!n) return 2;
  zh_ctx* ctx = nullptr;
  if (zh_create(0, nullptr, &ctx)) return 3;
  std::vector<const void*> ptrs(n);
  std::vector<size_t> lens(n);
  for (size_t i = 0; i < n; i++) {
    ptrs[i] = images[i].data();
    lens[i] = images[i].size();
  }
  int bad = 0;
  unsigned long sum = 0;
  for (int pass = 0; pass < 2; pass++) {  // each by itself, then all in one call
    for (size_t i0 = 0; i0 < n; i0 += pass ? n : 1) {
      const size_t m = pass ? n : 1;
      std::vector<zh_zip_reader*> rd(m);
      std::vector<int32_t> st(m);
      if (zh_zip_read_batch(ctx, ptrs.data() + i0, lens.data() + i0, m, rd.data(), st.data())) return 4;
      for (size_t k = 0; k < m; k++) {
        const int w = want[i0 + k];
        const bool as_expected = w >= 0 ? st[k] == w : st[k] > 0 && st[k] < ZH_ERR_ARCHIVE_EOF;
        if (!as_expected || (st[k] == ZH_OK) != (rd[k] != nullptr)) {
          fprintf(stderr, "image %zu (pass %d): status %d, expected %d\n", i0 + k, pass, st[k], w);
          bad++;
        }
        if (rd[k] && check_reader(ctx, rd[k], &sum)) bad++;
        zh_zip_close(rd[k]);
      }
    }
  }
  zh_destroy(ctx);
  printf("%s: %zu images, checksum %lu\n", bad ? "FAILED" : "sanitized zip read ok", n, sum);
  return bad ? 1 : 0;
}
