// Stand-alone driver for the host side of zh_zip_open_all_batch under -fsanitize=address,undefined (built by
// tests/test_zip_open_sanitize.py from zippy_amd/csrc against the emulator runtime of tests/hipemu): opens the images
// of a directory (NAME.zip, with expected.txt: "NAME.zip STATUS" a line) each by itself and all in one call, holds
// the archive statuses against the expected ones and against zh_zip_open, and reads every extracted byte.
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "../include/zippy_hip.h"

static int check_reader(zh_zip_reader* r, unsigned long* sum) {
  const size_t n = zh_zip_num_entries(r);
  for (size_t i = 0; i < n; i++) {
    zh_zip_entry e;
    const void* data;
    size_t len;
    int32_t st;
    if (zh_zip_entry_at(r, i, &e) || zh_zip_entry_data(r, i, &data, &len, &st)) return 1;
    for (size_t k = 0; k < e.path_len; k++) *sum += (unsigned char)e.path[k];
    if (st == ZH_OK)
      for (size_t k = 0; k < len; k++) *sum += ((const unsigned char*)data)[k];
  }
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
      if (zh_zip_open_all_batch(ctx, ptrs.data() + i0, lens.data() + i0, m, rd.data(), st.data())) return 4;
      for (size_t k = 0; k < m; k++) {
        zh_zip_reader* alone = nullptr;
        const int open_st = zh_zip_open(ptrs[i0 + k], lens[i0 + k], &alone);
        if (st[k] != want[i0 + k] || (open_st != ZH_OK) != (rd[k] == nullptr) || (open_st && open_st != st[k])) {
          fprintf(stderr, "image %zu (pass %d): status %d, expected %d, zh_zip_open %d\n", i0 + k, pass, st[k], want[i0 + k],
                  open_st);
          bad++;
        }
        if (rd[k] && check_reader(rd[k], &sum)) bad++;
        zh_zip_close(alone);
        zh_zip_close(rd[k]);
      }
    }
  }
  zh_destroy(ctx);
  printf("%s: %zu images, checksum %lu\n", bad ? "FAILED" : "sanitized zip open ok", n, sum);
  return bad ? 1 : 0;
}
