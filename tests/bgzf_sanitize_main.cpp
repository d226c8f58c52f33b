// Stand-alone driver for zh_bgzf_* under -fsanitize=address,undefined (built by tests/test_bgzf_sanitize.py from
// zippy_amd/csrc against the emulator runtime of tests/hipemu).  The directory holds what tests/bgzf_cases.py dumped:
//   write.txt     "NAME LEVEL BLOCK" a line: NAME.src is written and must equal NAME.bgzf, all of a (LEVEL, BLOCK) in one call
//   expected.txt  "NAME STATUS EOF" a line (-1: a status of the decoder's): NAME.bgzf is read and indexed, each by itself
//                 and all in one call; NAME.out is its data where STATUS is 0, NAME.idx its index ("COFF UOFF" a line)
//   ranges.txt    "IMAGE OFF LEN STATUS" a line, IMAGE a position in images.txt ("NAME": NAME.bgzf, NAME.idx the index
//                 to use -- it need not be sound --, NAME.src the data the ranges are slices of): all in one call
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iterator>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../include/zippy_hip.h"

static std::string slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
static std::vector<zh_bgzf_entry> read_index(const std::string& path) {
  std::ifstream f(path);
  std::vector<zh_bgzf_entry> out;
  unsigned long long c, u;
  while (f >> c >> u) out.push_back(zh_bgzf_entry{c, u});
  return out;
}
static bool as_expected(int want, int got) { return want >= 0 ? got == want : got > 0 && got < ZH_ERR_NOMEM; }

static int bad = 0;
#define EXPECT(cond, ...)            \
  do {                               \
    if (!(cond)) {                   \
      fprintf(stderr, __VA_ARGS__);  \
      fprintf(stderr, "\n");         \
      bad++;                         \
    }                                \
  } while (0)

static void run_write(zh_ctx* ctx, const std::string& dir) {
  std::ifstream list(dir + "/write.txt");
  std::map<std::pair<int, long>, std::vector<std::string>> calls;
  std::string name;
  int level;
  long block;
  while (list >> name >> level >> block) calls[{level, block}].push_back(name);
  for (const auto& c : calls) {
    const size_t n = c.second.size();
    std::vector<std::string> src(n), want(n);
    std::vector<const void*> ptrs(n);
    std::vector<size_t> lens(n), dlen(n);
    std::vector<void*> dst(n);
    std::vector<int32_t> st(n);
    for (size_t i = 0; i < n; i++) {
      src[i] = slurp(dir + "/" + c.second[i] + ".src");
      want[i] = slurp(dir + "/" + c.second[i] + ".bgzf");
      ptrs[i] = src[i].data();
      lens[i] = src[i].size();
    }
    const int rc = zh_bgzf_write_batch(ctx, ptrs.data(), lens.data(), n, c.first.first, (size_t)c.first.second,
                                       dst.data(), dlen.data(), st.data());
    EXPECT(rc == ZH_OK, "write (%d, %ld): call status %d", c.first.first, c.first.second, rc);
    for (size_t i = 0; i < n && rc == ZH_OK; i++) {
      EXPECT(st[i] == ZH_OK && dst[i] && dlen[i] == want[i].size() && !memcmp(dst[i], want[i].data(), dlen[i]),
             "write %s: status %d, %zu bytes for %zu", c.second[i].c_str(), st[i], dlen[i], want[i].size());
      zh_free(dst[i]);
    }
  }
  // the call errors: nothing is handed out
  const char* s = "abc";
  const void* p = s;
  size_t len = 3, dl = 7;
  void* d = (void*)s;
  int32_t st = 5;
  EXPECT(zh_bgzf_write_batch(ctx, &p, &len, 1, 10, 0, &d, &dl, &st) == ZH_ERR_INVALID_LEVEL && !d && !dl &&
             st == ZH_ERR_INVALID_LEVEL, "write: level 10");
  EXPECT(zh_bgzf_write_batch(ctx, &p, &len, 1, 1, ZH_BGZF_MAX_BLOCK + 1, &d, &dl, &st) == ZH_ERR_ARGUMENT && !d,
         "write: block_bytes beyond the largest");
  EXPECT(zh_bgzf_write_batch(ctx, nullptr, nullptr, 0, 1, 0, nullptr, nullptr, nullptr) == ZH_OK, "write: no image");
}

static void run_read(zh_ctx* ctx, const std::string& dir, unsigned long* sum) {
  std::ifstream list(dir + "/expected.txt");
  std::vector<std::string> names, images;
  std::vector<int> want, want_eof;
  std::string name;
  int status, eof;
  while (list >> name >> status >> eof) {
    names.push_back(name);
    images.push_back(slurp(dir + "/" + name + ".bgzf"));
    want.push_back(status);
    want_eof.push_back(eof);
  }
  const size_t n = images.size();
  EXPECT(n > 0, "no images");
  std::vector<const void*> ptrs(n);
  std::vector<size_t> lens(n);
  for (size_t i = 0; i < n; i++) {
    ptrs[i] = images[i].data();
    lens[i] = images[i].size();
  }
  for (int pass = 0; pass < 2; pass++) {  // each by itself, then all in one call
    for (size_t i0 = 0; i0 < n; i0 += pass ? n : 1) {
      const size_t m = pass ? n : 1;
      std::vector<void*> dst(m);
      std::vector<size_t> dlen(m), first(m + 1);
      std::vector<int32_t> st(m), ist(m);
      std::vector<uint8_t> he(m), ihe(m);
      zh_bgzf_entry* index = nullptr;
      const int rc = zh_bgzf_read_batch(ctx, ptrs.data() + i0, lens.data() + i0, m, dst.data(), dlen.data(), st.data(),
                                        pass ? he.data() : nullptr);
      const int irc = zh_bgzf_index_batch(ctx, ptrs.data() + i0, lens.data() + i0, m, &index, first.data(), ist.data(),
                                          ihe.data());
      EXPECT(rc == ZH_OK && irc == ZH_OK, "read / index: call status %d / %d", rc, irc);
      if (rc || irc) continue;
      for (size_t k = 0; k < m; k++) {
        const size_t i = i0 + k;
        EXPECT(as_expected(want[i], st[k]) && (st[k] == ZH_OK) == (dst[k] != nullptr),
               "read %s (pass %d): status %d, expected %d", names[i].c_str(), pass, st[k], want[i]);
        EXPECT(ihe[k] == want_eof[i] && (!pass || he[k] == want_eof[i]), "%s: has_eof", names[i].c_str());
        if (st[k] == ZH_OK) {
          const std::string out = slurp(dir + "/" + names[i] + ".out");
          EXPECT(dlen[k] == out.size() && !memcmp(dst[k], out.data(), dlen[k]), "read %s: the data", names[i].c_str());
          for (size_t j = 0; j < dlen[k]; j++) *sum += ((const unsigned char*)dst[k])[j];
        }
        const std::vector<zh_bgzf_entry> widx = read_index(dir + "/" + names[i] + ".idx");
        EXPECT((ist[k] == ZH_OK) == !widx.empty() && first[k + 1] - first[k] == widx.size(),
               "index %s: status %d, %zu entries for %zu", names[i].c_str(), ist[k], first[k + 1] - first[k], widx.size());
        for (size_t j = 0; j < widx.size() && first[k + 1] - first[k] == widx.size(); j++)
          EXPECT(index[first[k] + j].coff == widx[j].coff && index[first[k] + j].uoff == widx[j].uoff, "index %s: entry %zu",
                 names[i].c_str(), j);
        zh_free(dst[k]);
      }
      zh_free(index);
    }
  }
}

static void run_ranges(zh_ctx* ctx, const std::string& dir, unsigned long* sum) {
  std::ifstream list(dir + "/images.txt");
  std::vector<std::string> images, srcs;
  std::vector<zh_bgzf_entry> index;
  std::vector<size_t> first{0};
  std::string name;
  while (list >> name) {
    images.push_back(slurp(dir + "/" + name + ".bgzf"));
    srcs.push_back(slurp(dir + "/" + name + ".src"));
    for (const zh_bgzf_entry& e : read_index(dir + "/" + name + ".idx")) index.push_back(e);
    first.push_back(index.size());
  }
  const size_t n = images.size();
  std::vector<const void*> ptrs(n);
  std::vector<size_t> lens(n);
  for (size_t i = 0; i < n; i++) {
    ptrs[i] = images[i].data();
    lens[i] = images[i].size();
  }
  std::ifstream rl(dir + "/ranges.txt");
  std::vector<uint64_t> ri, ro, rn;
  std::vector<int> want;
  unsigned long long a, b, c;
  int status;
  while (rl >> a >> b >> c >> status) {
    ri.push_back(a);
    ro.push_back(b);
    rn.push_back(c);
    want.push_back(status);
  }
  const size_t nr = ri.size();
  EXPECT(n > 0 && nr > 0, "no ranges");
  std::vector<void*> dst(nr);
  std::vector<size_t> dlen(nr);
  std::vector<int32_t> st(nr);
  const int rc = zh_bgzf_read_ranges(ctx, ptrs.data(), lens.data(), n, index.data(), first.data(), nr, ri.data(),
                                     ro.data(), rn.data(), dst.data(), dlen.data(), st.data());
  EXPECT(rc == ZH_OK, "ranges: call status %d", rc);
  for (size_t r = 0; r < nr && rc == ZH_OK; r++) {
    EXPECT(as_expected(want[r], st[r]) && (st[r] == ZH_OK) == (dst[r] != nullptr), "range %zu: status %d, expected %d", r,
           st[r], want[r]);
    if (st[r] == ZH_OK) {
      const std::string& s = srcs[ri[r]];
      const size_t lo = ro[r] < s.size() ? (size_t)ro[r] : s.size();
      const size_t len = rn[r] < s.size() - lo ? (size_t)rn[r] : s.size() - lo;
      EXPECT(dlen[r] == len && !memcmp(dst[r], s.data() + lo, len), "range %zu: the data", r);
      for (size_t j = 0; j < dlen[r]; j++) *sum += ((const unsigned char*)dst[r])[j];
    }
    zh_free(dst[r]);
  }
  uint64_t bad_image = n, one = 1;
  void* d = nullptr;
  size_t dl = 0;
  int32_t s1 = 0;
  EXPECT(zh_bgzf_read_ranges(ctx, ptrs.data(), lens.data(), n, index.data(), first.data(), 1, &bad_image, &one, &one, &d,
                             &dl, &s1) == ZH_ERR_ARGUMENT && !d, "ranges: an image that is not there");
  uint64_t up = 0, ip = 0, sc = 0;
  EXPECT(zh_debug_range_stats(ctx, &up, &ip, &sc) == ZH_OK && up > 0 && ip + sc > 0, "ranges: the counters");
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  zh_ctx* ctx = nullptr;
  if (zh_create(0, nullptr, &ctx)) return 3;
  unsigned long sum = 0;
  run_write(ctx, dir);
  run_read(ctx, dir, &sum);
  run_ranges(ctx, dir, &sum);
  zh_destroy(ctx);
  printf("%s: checksum %lu\n", bad ? "FAILED" : "sanitized bgzf ok", sum);
  return bad ? 1 : 0;
}
