// Stand-alone driver for the host side of zh_tar_read_batch under -fsanitize=address,undefined (built by
// tests/test_tar_read_sanitize.py from zippy_amd/csrc against the emulator runtime of tests/hipemu): opens the images
// of a directory (NAME.tar, with expected.txt: "NAME.tar FORMAT STATUS" a line; -1: a status of the decoder's) each
// by itself and all in one call, holds the statuses against the expected ones, and reads every field and byte of
// every reader.
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../include/zippy_hip.h"

static int check_reader(zh_tar_reader* r, unsigned long* sum) {
  size_t len = 0;
  const unsigned char* data = (const unsigned char*)zh_tar_data(r, &len);
  const size_t n = zh_tar_num_entries(r);
  for (size_t i = 0; i < n; i++) {
    zh_tar_entry e;
    if (zh_tar_entry_at(r, i, &e) || e.linkname_len != 0 || (e.typeflag != '0' && e.typeflag != '5')) return 1;
    if (e.offset + e.size > len) return 1;
    if (e.typeflag == '5' && (e.offset || e.size || e.mode || e.mtime)) return 1;
    for (size_t k = 0; k < e.path_len; k++) *sum += (unsigned char)e.path[k];
    for (uint64_t k = 0; k < e.size; k++) *sum += data[e.offset + k];
    *sum += e.mode + (unsigned long)e.mtime;
  }
  zh_tar_entry e;
  if (zh_tar_entry_at(r, n, &e) == ZH_OK) return 1;
  if (len) *sum += data[0] + data[len - 1];
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  std::ifstream list(dir + "/expected.txt");
  std::vector<std::string> images;
  std::vector<int32_t> formats;
  std::vector<int> want;
  std::string name;
  int format, status;
  while (list >> name >> format >> status) {
    std::ifstream f(dir + "/" + name, std::ios::binary);
    images.emplace_back(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    formats.push_back(format);
    want.push_back(status);
  }
  const size_t n = images.size();
  if (!n) return 2;
  zh_ctx* ctx = nullptr;
  if (zh_create(0, nullptr, &ctx)) return 3;
  std::vector<const void*> ptrs(n);
  std::vector<size_t> lens(n);
  for (size_t i = 0; i < n; i++) {
    ptrs[i] = images[i].empty() ? nullptr : images[i].data();
    lens[i] = images[i].size();
  }
  int bad = 0;
  unsigned long sum = 0;
  for (int pass = 0; pass < 2; pass++) {  // each by itself, then all in one call
    for (size_t i0 = 0; i0 < n; i0 += pass ? n : 1) {
      const size_t m = pass ? n : 1;
      std::vector<zh_tar_reader*> rd(m);
      std::vector<int32_t> st(m);
      if (zh_tar_read_batch(ctx, ptrs.data() + i0, lens.data() + i0, formats.data() + i0, m, rd.data(), st.data()))
        return 4;
      for (size_t k = 0; k < m; k++) {
        const int w = want[i0 + k];
        const bool as_expected = w >= 0 ? st[k] == w : st[k] > 0 && st[k] < ZH_ERR_ARGUMENT;
        if (!as_expected || (st[k] == ZH_OK) != (rd[k] != nullptr)) {
          fprintf(stderr, "image %zu (pass %d): status %d, expected %d\n", i0 + k, pass, st[k], w);
          bad++;
        }
        if (rd[k] && check_reader(rd[k], &sum)) bad++;
        zh_tar_close(rd[k]);
      }
    }
  }
  // formats == NULL: all detect; a format outside 0..2: the call's own error, the outputs cleared
  {
    std::vector<zh_tar_reader*> rd(n);
    std::vector<int32_t> st(n);
    if (zh_tar_read_batch(ctx, ptrs.data(), lens.data(), nullptr, n, rd.data(), st.data())) return 5;
    for (size_t k = 0; k < n; k++) {
      if (formats[k] == ZH_TF_DETECT && st[k] != (want[k] >= 0 ? want[k] : st[k])) bad++;
      if (rd[k] && check_reader(rd[k], &sum)) bad++;
      zh_tar_close(rd[k]);
    }
    formats[n - 1] = 3;
    if (zh_tar_read_batch(ctx, ptrs.data(), lens.data(), formats.data(), n, rd.data(), st.data()) != ZH_ERR_ARGUMENT)
      bad++;
    for (size_t k = 0; k < n; k++)
      if (rd[k] || st[k]) bad++;
  }
  zh_destroy(ctx);
  printf("%s: %zu images, checksum %lu\n", bad ? "FAILED" : "sanitized tar read ok", n, sum);
  return bad ? 1 : 0;
}
