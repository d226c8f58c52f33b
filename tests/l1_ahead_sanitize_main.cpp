// Stand-alone driver for the BestSpeed matcher under -fsanitize=address,undefined (built by
// tests/test_l1_ahead_sanitize.py from zippy_amd/csrc against the emulator runtime of tests/hipemu, whose device
// allocations are plain malloc blocks the sanitizer guards): every input of a directory (NAME, listed in list.txt)
// is compressed at level 1 from a device allocation of its own that ends with the dword that holds the input's last
// byte -- the matcher reads its source as aligned dwords, "never past the dword that holds its last byte" -- with the
// input 0, 1, 2 and 3 bytes behind the allocation's start: for every length one of the four ends exactly with the
// last byte.  All inputs of one misalignment go through ONE plan: their offsets are the distances of their blocks
// from the lowest one.  The streams are held against expected/NAME (raw deflate, the oracle's).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../include/zippy_hip.h"

static std::string slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  std::ifstream list(dir + "/list.txt");
  std::vector<std::string> src, want;
  std::string name;
  while (list >> name) {
    src.push_back(slurp(dir + "/" + name));
    want.push_back(slurp(dir + "/expected/" + name));
  }
  const size_t n = src.size();
  if (!n) return 2;
  zh_ctx* ctx = nullptr;
  if (zh_create(0, nullptr, &ctx)) return 3;
  int bad = 0;
  size_t total = 0;
  for (unsigned mis = 0; mis < 4; mis++) {
    std::vector<unsigned char*> blocks(n);
    for (size_t i = 0; i < n; i++) {
      const size_t bytes = (mis + src[i].size() + 3) & ~(size_t)3;
      blocks[i] = (unsigned char*)malloc(bytes ? bytes : 1);
      if (!blocks[i]) return 4;
      memcpy(blocks[i] + mis, src[i].data(), src[i].size());
    }
    const unsigned char* base = *std::min_element(blocks.begin(), blocks.end());
    std::vector<uint64_t> src_off(n), src_len(n), dst_off(n), dst_cap(n);
    uint64_t at = 0;
    for (size_t i = 0; i < n; i++) {
      src_off[i] = (uint64_t)(blocks[i] + mis - base);
      src_len[i] = src[i].size();
      dst_off[i] = at;
      dst_cap[i] = src[i].size() + src[i].size() / 8 + 256;
      at += (dst_cap[i] + 255) & ~(uint64_t)255;
    }
    unsigned char* dst = (unsigned char*)malloc(at);
    zh_plan* plan = nullptr;
    if (zh_plan_compress(ctx, n, src_off.data(), src_len.data(), dst_off.data(), dst_cap.data(), 1, ZH_DF_DEFLATE, &plan))
      return 5;
    std::vector<uint64_t> lens(n);
    std::vector<int32_t> st(n);
    if (zh_plan_run(plan, base, dst) || zh_plan_results(plan, lens.data(), st.data())) return 6;
    for (size_t i = 0; i < n; i++) {
      if (st[i] != ZH_OK || lens[i] != want[i].size() || memcmp(dst + dst_off[i], want[i].data(), lens[i]) != 0) {
        fprintf(stderr, "input %zu at misalignment %u: status %d, %llu bytes, expected %zu\n", i, mis, st[i],
                (unsigned long long)lens[i], want[i].size());
        bad++;
      }
      total += lens[i];
    }
    zh_plan_destroy(plan);
    free(dst);
    for (size_t i = 0; i < n; i++) free(blocks[i]);
  }
  zh_destroy(ctx);
  printf("%s: %zu inputs x 4 misalignments, %zu bytes of deflate\n", bad ? "FAILED" : "sanitized l1 match ok", n, total);
  return bad ? 1 : 0;
}
