// Stand-alone driver for zh_gzip_read_batch under -fsanitize=address,undefined (built by tests/test_gzip_sanitize.py
// from zippy_amd/csrc against the emulator runtime of tests/hipemu).  The directory holds what tests/gzip_cases.py
// dumped:
//   cases.txt     "NAME IMAGES BUDGET" a line; BUDGET: ZH_GZIP_SPEC_BYTES for the case (-1: the default)
//   NAME_<i>.bin  image i, .out its data, .mem its members as zh_gzip_member records
//   NAME.st       a status a line (-1: any status but ZH_OK)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../include/zippy_hip.h"

static std::string slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

static int bad = 0;
#define EXPECT(cond, ...)            \
  do {                               \
    if (!(cond)) {                   \
      fprintf(stderr, __VA_ARGS__);  \
      fprintf(stderr, "\n");         \
      bad++;                         \
    }                                \
  } while (0)

static void run_case(zh_ctx* ctx, const std::string& dir, const std::string& name, size_t n, long long budget, int mode,
                     unsigned long* sum) {
  std::vector<std::string> images(n), outs(n), mems(n);
  std::vector<int> want;
  for (size_t i = 0; i < n; i++) {
    const std::string base = dir + "/" + name + "_" + std::to_string(i);
    // (every image in an allocation of exactly its size, at an odd address: reads past it are the sanitizer's to find)
    images[i] = slurp(base + ".bin");
    outs[i] = slurp(base + ".out");
    mems[i] = slurp(base + ".mem");
  }
  std::ifstream f(dir + "/" + name + ".st");
  int status;
  while (f >> status) want.push_back(status);
  EXPECT(want.size() == n, "%s: %zu statuses for %zu images", name.c_str(), want.size(), n);
  if (want.size() != n) return;
  if (budget >= 0)
    setenv("ZH_GZIP_SPEC_BYTES", std::to_string(budget).c_str(), 1);
  else
    unsetenv("ZH_GZIP_SPEC_BYTES");
  std::vector<std::vector<char>> held(n);
  std::vector<const void*> ptrs(n);
  std::vector<size_t> lens(n), dlen(n, 7), first(n + 1, 7);
  for (size_t i = 0; i < n; i++) {
    held[i].assign(images[i].begin(), images[i].end());
    ptrs[i] = held[i].empty() ? nullptr : held[i].data();
    lens[i] = held[i].size();
  }
  std::vector<void*> dst(n, &bad);
  std::vector<int32_t> st(n, 5);
  zh_gzip_member* mem = nullptr;
  const bool data = mode != 1, members = mode != 2;
  const int rc = zh_gzip_read_batch(ctx, ptrs.data(), lens.data(), n, data ? dst.data() : nullptr, data ? dlen.data() : nullptr,
                                    st.data(), members ? &mem : nullptr, members ? first.data() : nullptr);
  EXPECT(rc == ZH_OK, "%s: call status %d", name.c_str(), rc);
  if (rc) return;
  for (size_t i = 0; i < n; i++) {
    EXPECT(want[i] >= 0 ? st[i] == want[i] : st[i] != ZH_OK, "%s image %zu: status %d, expected %d", name.c_str(), i, st[i], want[i]);
    if (data) {
      EXPECT((st[i] == ZH_OK) == (dst[i] != nullptr), "%s image %zu: data of a status %d", name.c_str(), i, st[i]);
      if (st[i] == ZH_OK && dst[i]) {
        EXPECT(dlen[i] == outs[i].size() && !memcmp(dst[i], outs[i].data(), dlen[i]), "%s image %zu: the data", name.c_str(), i);
        for (size_t j = 0; j < dlen[i]; j++) *sum += ((const unsigned char*)dst[i])[j];
      }
      zh_free(dst[i]);
    }
    if (members) {
      const size_t k = first[i + 1] - first[i];
      EXPECT(first[i + 1] >= first[i] && k * sizeof(zh_gzip_member) == (st[i] == ZH_OK ? mems[i].size() : 0),
             "%s image %zu: %zu members", name.c_str(), i, k);
      if (st[i] == ZH_OK && k * sizeof(zh_gzip_member) == mems[i].size())
        EXPECT(!k || !memcmp(mem + first[i], mems[i].data(), mems[i].size()), "%s image %zu: the members", name.c_str(), i);
    }
  }
  if (budget > 0) {
    uint64_t cand = 0, spec = 0, rounds = 0;
    EXPECT(zh_debug_gzip_stats(ctx, &cand, &spec, &rounds) == ZH_OK && cand > 0 && rounds > 0 && spec >= (uint64_t)budget &&
               spec <= (uint64_t)budget + 65540,  // (one workgroup at a time: one look's worth, a full stored block at most)
           "%s: %llu candidates, %llu bytes, %llu rounds", name.c_str(), (unsigned long long)cand, (unsigned long long)spec,
           (unsigned long long)rounds);
  }
  zh_free(mem);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  zh_ctx* ctx = nullptr;
  if (zh_create(0, nullptr, &ctx)) return 3;
  unsigned long sum = 0;
  std::ifstream list(dir + "/cases.txt");
  std::string name;
  size_t n, n_cases = 0;
  long long budget;
  while (list >> name >> n >> budget) {
    run_case(ctx, dir, name, n, budget, (int)(n_cases % 3), &sum);
    n_cases++;
  }
  EXPECT(n_cases > 0, "no cases");
  unsetenv("ZH_GZIP_SPEC_BYTES");
  // the call errors: nothing is handed out
  const void* src = "x";
  size_t len = 1, dl = 7, first[2] = {7, 7};
  void* d = &len;
  int32_t st = 5;
  zh_gzip_member* mem = (zh_gzip_member*)&len;
  EXPECT(zh_gzip_read_batch(ctx, nullptr, &len, 1, &d, &dl, &st, nullptr, nullptr) == ZH_ERR_ARGUMENT, "gzip: no images");
  EXPECT(zh_gzip_read_batch(ctx, &src, &len, 1, &d, nullptr, &st, nullptr, nullptr) == ZH_ERR_ARGUMENT, "gzip: dsts without dst_lens");
  EXPECT(zh_gzip_read_batch(ctx, &src, &len, 1, &d, &dl, &st, &mem, nullptr) == ZH_ERR_ARGUMENT, "gzip: members without first");
  EXPECT(zh_gzip_read_batch(ctx, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == ZH_OK, "gzip: no image");
  EXPECT(zh_gzip_read_batch(ctx, &src, &len, 1, &d, &dl, &st, &mem, first) == ZH_OK && st == ZH_ERR_INVALID_BUFFER && !d && !dl &&
             mem && first[0] == 0 && first[1] == 0, "gzip: one byte");
  zh_free(mem);
  zh_destroy(ctx);
  printf("%s: checksum %lu\n", bad ? "FAILED" : "sanitized gzip ok", sum);
  return bad ? 1 : 0;
}
