// Stand-alone driver for zh_seek_index_batch and zh_seek_read_ranges under -fsanitize=address,undefined (built by
// tests/test_seek_sanitize.py from zippy_amd/csrc against the emulator runtime of tests/hipemu).  The directory holds
// what tests/seek_cases.py dumped:
//   cases.txt     "NAME STREAMS FORMAT SPAN" a line; FORMAT -1: the streams are read only, no index is built
//   NAME_<s>.bin  stream s, .src its plaintext, .blob the blob the build must give (empty: none, and a status that is
//                 not ZH_OK), .rblob the blob the ranges are read with (it need not be sound)
//   NAME.ranges   "STREAM OFF LEN STATUS" a line (-1: any status but ZH_OK and ZH_ERR_CHECKSUM)
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
static bool as_expected(int want, int got) { return want >= 0 ? got == want : got != ZH_OK && got != ZH_ERR_CHECKSUM; }

static int bad = 0;
#define EXPECT(cond, ...)            \
  do {                               \
    if (!(cond)) {                   \
      fprintf(stderr, __VA_ARGS__);  \
      fprintf(stderr, "\n");         \
      bad++;                         \
    }                                \
  } while (0)

struct Case {
  std::string name;
  int fmt = 0;
  unsigned long long span = 0;
  std::vector<std::string> streams, srcs, blobs, rblobs;
  std::vector<uint64_t> rs, ro, rl;
  std::vector<int> want;
};

static Case load(const std::string& dir, const std::string& name, size_t n_streams, int fmt, unsigned long long span) {
  Case c;
  c.name = name;
  c.fmt = fmt;
  c.span = span;
  for (size_t s = 0; s < n_streams; s++) {
    const std::string base = dir + "/" + name + "_" + std::to_string(s);
    c.streams.push_back(slurp(base + ".bin"));
    c.srcs.push_back(slurp(base + ".src"));
    c.blobs.push_back(slurp(base + ".blob"));
    c.rblobs.push_back(slurp(base + ".rblob"));
  }
  std::ifstream f(dir + "/" + name + ".ranges");
  unsigned long long a, b, n;
  int status;
  while (f >> a >> b >> n >> status) {
    c.rs.push_back(a);
    c.ro.push_back(b);
    c.rl.push_back(n);
    c.want.push_back(status);
  }
  return c;
}

static void run_build(zh_ctx* ctx, const Case& c, bool want_data, unsigned long* sum) {
  const size_t n = c.streams.size();
  std::vector<const void*> ptrs(n);
  std::vector<size_t> lens(n), ilen(n), dlen(n);
  for (size_t s = 0; s < n; s++) {
    ptrs[s] = c.streams[s].data();
    lens[s] = c.streams[s].size();
  }
  std::vector<void*> idx(n), dst(n);
  std::vector<int32_t> st(n);
  const int rc = zh_seek_index_batch(ctx, ptrs.data(), lens.data(), n, c.fmt, c.span, idx.data(), ilen.data(),
                                     want_data ? dst.data() : nullptr, want_data ? dlen.data() : nullptr, st.data());
  EXPECT(rc == ZH_OK, "%s: build status %d", c.name.c_str(), rc);
  if (rc) return;
  for (size_t s = 0; s < n; s++) {
    const bool sound = !c.blobs[s].empty();
    EXPECT((st[s] == ZH_OK) == sound && (idx[s] != nullptr) == sound, "%s stream %zu: build status %d", c.name.c_str(), s, st[s]);
    if (sound && idx[s])
      EXPECT(ilen[s] == c.blobs[s].size() && !memcmp(idx[s], c.blobs[s].data(), ilen[s]), "%s stream %zu: the blob", c.name.c_str(), s);
    if (want_data && sound)
      EXPECT(dst[s] && dlen[s] == c.srcs[s].size() && !memcmp(dst[s], c.srcs[s].data(), dlen[s]), "%s stream %zu: the data",
             c.name.c_str(), s);
    for (size_t j = 0; idx[s] && j < ilen[s]; j++) *sum += ((const unsigned char*)idx[s])[j];
    zh_free(idx[s]);
    if (want_data) zh_free(dst[s]);
  }
}

static void run_read(zh_ctx* ctx, const Case& c, unsigned long* sum) {
  const size_t n = c.streams.size(), nr = c.rs.size();
  std::vector<const void*> ptrs(n), iptrs(n);
  std::vector<size_t> lens(n), ilens(n), dlen(nr);
  // (the blobs at odd addresses: a caller keeps them wherever it likes)
  std::vector<std::string> odd(n);
  for (size_t s = 0; s < n; s++) {
    ptrs[s] = c.streams[s].data();
    lens[s] = c.streams[s].size();
    odd[s] = std::string(1 + s % 7, 'x') + c.rblobs[s];
    iptrs[s] = c.rblobs[s].empty() ? nullptr : odd[s].data() + 1 + s % 7;
    ilens[s] = c.rblobs[s].size();
  }
  std::vector<void*> dst(nr);
  std::vector<int32_t> st(nr);
  const int rc = zh_seek_read_ranges(ctx, ptrs.data(), lens.data(), n, iptrs.data(), ilens.data(), nr, c.rs.data(),
                                     c.ro.data(), c.rl.data(), dst.data(), dlen.data(), st.data());
  EXPECT(rc == ZH_OK, "%s: read status %d", c.name.c_str(), rc);
  if (rc) return;
  for (size_t r = 0; r < nr; r++) {
    EXPECT(as_expected(c.want[r], st[r]) && (st[r] == ZH_OK) == (dst[r] != nullptr), "%s range %zu: status %d, expected %d",
           c.name.c_str(), r, st[r], c.want[r]);
    if (st[r] == ZH_OK && dst[r]) {
      const std::string& s = c.srcs[c.rs[r]];
      const size_t lo = c.ro[r] < s.size() ? (size_t)c.ro[r] : s.size();
      const size_t len = c.rl[r] < s.size() - lo ? (size_t)c.rl[r] : s.size() - lo;
      EXPECT(dlen[r] == len && !memcmp(dst[r], s.data() + lo, len), "%s range %zu: the data", c.name.c_str(), r);
      for (size_t j = 0; j < dlen[r]; j++) *sum += ((const unsigned char*)dst[r])[j];
    }
    zh_free(dst[r]);
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  zh_ctx* ctx = nullptr;
  if (zh_create(0, nullptr, &ctx)) return 3;
  unsigned long sum = 0;
  std::ifstream list(dir + "/cases.txt");
  std::string name;
  size_t n_streams, n_cases = 0;
  int fmt;
  unsigned long long span;
  while (list >> name >> n_streams >> fmt >> span) {
    const Case c = load(dir, name, n_streams, fmt, span);
    EXPECT(!c.rs.empty(), "%s: no ranges", name.c_str());
    if (fmt >= 0) run_build(ctx, c, n_cases % 2 == 0, &sum);
    run_read(ctx, c, &sum);
    n_cases++;
  }
  EXPECT(n_cases > 0, "no cases");
  // the call errors: nothing is handed out
  uint64_t one = 1;
  size_t dl = 7, il = 7;
  void *d = &one, *ix = &one;
  const void* src = "x";
  size_t len = 1;
  int32_t st = 5;
  EXPECT(zh_seek_read_ranges(ctx, nullptr, nullptr, 0, nullptr, nullptr, 1, &one, &one, &one, &d, &dl, &st) == ZH_ERR_ARGUMENT &&
             !d && !dl && st == ZH_OK, "seek ranges: a stream that is not there");
  EXPECT(zh_seek_read_ranges(ctx, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                             nullptr) == ZH_OK, "seek ranges: no range");
  EXPECT(zh_seek_index_batch(ctx, &src, &len, 1, ZH_DF_GZIP, 100, &ix, &il, nullptr, nullptr, &st) == ZH_ERR_ARGUMENT && !ix && !il,
         "seek index: a span below the window");
  EXPECT(zh_seek_index_batch(ctx, nullptr, nullptr, 0, ZH_DF_GZIP, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == ZH_OK,
         "seek index: no stream");
  zh_destroy(ctx);
  printf("%s: checksum %lu\n", bad ? "FAILED" : "sanitized seek ok", sum);
  return bad ? 1 : 0;
}
