// Stand-alone driver for zh_uncompress_ranges and zh_plan_uncompress_ranges + zh_plan_run under
// -fsanitize=address,undefined (built by tests/test_ranges_sanitize.py from zippy_amd/csrc against the emulator runtime
// of tests/hipemu).  The directory holds what tests/ranges_cases.py dumped:
//   cases.txt     "NAME STREAMS U" a line: one call of each form a case; U >= 0: the host call's upload lies between
//                 U and U + 15 bytes a range
//   NAME_<s>.bin  stream s, NAME_<s>.idx its index ("BIT_OFF OUT_OFF" a line -- it need not be sound), NAME_<s>.src
//                 the data the ranges are slices of
//   NAME.ranges   "STREAM OFF LEN STATUS" a line (-1: a status of the decoder's)
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

struct Case {
  std::string name;
  std::vector<std::string> streams, srcs;
  std::vector<zh_block_entry> index;
  std::vector<size_t> first{0};
  std::vector<uint64_t> rs, ro, rl;
  std::vector<int> want;
  long long U = -1;
  // the slice a range asks for
  const char* slice(size_t r, size_t* len) const {
    const std::string& s = srcs[rs[r]];
    const size_t lo = ro[r] < s.size() ? (size_t)ro[r] : s.size();
    *len = rl[r] < s.size() - lo ? (size_t)rl[r] : s.size() - lo;
    return s.data() + lo;
  }
};

static Case load(const std::string& dir, const std::string& name, size_t n_streams, long long U) {
  Case c;
  c.name = name;
  c.U = U;
  for (size_t s = 0; s < n_streams; s++) {
    const std::string base = dir + "/" + name + "_" + std::to_string(s);
    c.streams.push_back(slurp(base + ".bin"));
    c.srcs.push_back(slurp(base + ".src"));
    std::ifstream f(base + ".idx");
    unsigned long long bit, out;
    while (f >> bit >> out) c.index.push_back(zh_block_entry{bit, out});
    c.first.push_back(c.index.size());
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

static void run_host(zh_ctx* ctx, const Case& c, unsigned long* sum) {
  const size_t n = c.streams.size(), nr = c.rs.size();
  std::vector<const void*> ptrs(n);
  std::vector<size_t> lens(n), dlen(nr);
  for (size_t s = 0; s < n; s++) {
    ptrs[s] = c.streams[s].data();
    lens[s] = c.streams[s].size();
  }
  std::vector<void*> dst(nr);
  std::vector<int32_t> st(nr);
  const int rc = zh_uncompress_ranges(ctx, ptrs.data(), lens.data(), n, c.index.data(), c.first.data(), nr, c.rs.data(),
                                      c.ro.data(), c.rl.data(), dst.data(), dlen.data(), st.data());
  EXPECT(rc == ZH_OK, "%s: call status %d", c.name.c_str(), rc);
  if (rc) return;
  for (size_t r = 0; r < nr; r++) {
    EXPECT(as_expected(c.want[r], st[r]) && (st[r] == ZH_OK) == (dst[r] != nullptr), "%s range %zu: status %d, expected %d",
           c.name.c_str(), r, st[r], c.want[r]);
    if (st[r] == ZH_OK) {
      size_t len;
      const char* w = c.slice(r, &len);
      EXPECT(dlen[r] == len && !memcmp(dst[r], w, len), "%s range %zu: the data", c.name.c_str(), r);
      for (size_t j = 0; j < dlen[r]; j++) *sum += ((const unsigned char*)dst[r])[j];
    }
    zh_free(dst[r]);
  }
  uint64_t up = 0;
  EXPECT(zh_debug_range_stats(ctx, &up, nullptr, nullptr) == ZH_OK, "%s: the counters", c.name.c_str());
  if (c.U >= 0)
    EXPECT((uint64_t)c.U <= up && up <= (uint64_t)c.U + 15 * nr, "%s: %llu bytes uploaded for a union of %lld", c.name.c_str(),
           (unsigned long long)up, c.U);
}

// The device form: the streams at 256-byte steps with odd bytes in front, the slots exactly as long as the slices,
// at odd offsets, 48 guard bytes apart in a destination of 0xA5 -- every byte of which is held against what it must be
// but for the slot of a range that failed on a block, which is unspecified.
static void run_plan(zh_ctx* ctx, const Case& c, unsigned long* sum) {
  const size_t n = c.streams.size(), nr = c.rs.size();
  std::string img;
  std::vector<uint64_t> soff(n), slen(n), doff(nr), dcap(nr);
  for (size_t s = 0; s < n; s++) {
    img.append((256 - img.size() % 256) % 256 + s % 4, '\xee');
    soff[s] = img.size();
    slen[s] = c.streams[s].size();
    img += c.streams[s];
  }
  img.append(16, '\xee');
  size_t at = 64 + 3;
  for (size_t r = 0; r < nr; r++) {
    size_t len;
    (void)c.slice(r, &len);
    doff[r] = at;
    dcap[r] = len;
    at += (len + 15) / 16 * 16 + 48;
  }
  const size_t dst_size = at + 64;
  std::string want(dst_size, '\xa5'), got(dst_size, '\0');
  std::vector<char> loose(dst_size, 0);
  void *d_src = nullptr, *d_dst = nullptr;
  zh_plan* plan = nullptr;
  std::vector<uint64_t> olen(nr);
  std::vector<int32_t> st(nr);
  int rc = zh_device_malloc(ctx, img.size(), &d_src);
  if (!rc) rc = zh_device_malloc(ctx, dst_size, &d_dst);
  if (!rc) rc = zh_device_upload(ctx, d_src, img.data(), img.size());
  if (!rc) rc = zh_device_upload(ctx, d_dst, want.data(), dst_size);
  if (!rc)
    rc = zh_plan_uncompress_ranges(ctx, n, soff.data(), slen.data(), c.index.data(), c.first.data(), nr, c.rs.data(),
                                   c.ro.data(), c.rl.data(), doff.data(), dcap.data(), &plan);
  if (!rc) rc = zh_plan_run(plan, d_src, d_dst);
  if (!rc) rc = zh_plan_results(plan, olen.data(), st.data());
  if (!rc) rc = zh_device_download(ctx, &got[0], d_dst, dst_size);
  EXPECT(rc == ZH_OK, "%s: the plan, status %d", c.name.c_str(), rc);
  for (size_t r = 0; r < nr && rc == ZH_OK; r++) {
    size_t len;
    const char* w = c.slice(r, &len);
    EXPECT(as_expected(c.want[r], st[r]), "%s plan range %zu: status %d, expected %d", c.name.c_str(), r, st[r], c.want[r]);
    if (st[r] == ZH_OK) {
      EXPECT(olen[r] == len, "%s plan range %zu: %llu bytes for %zu", c.name.c_str(), r, (unsigned long long)olen[r], len);
      memcpy(&want[doff[r]], w, len);
    } else {
      EXPECT(olen[r] == 0, "%s plan range %zu: a length with status %d", c.name.c_str(), r, st[r]);
      memset(&loose[doff[r]], 1, len);
    }
  }
  for (size_t i = 0; i < dst_size && rc == ZH_OK; i++) {
    if (!loose[i] && got[i] != want[i]) {
      EXPECT(false, "%s plan: destination byte %zu", c.name.c_str(), i);
      break;
    }
    *sum += (unsigned char)got[i] * (loose[i] ? 0u : 1u);
  }
  zh_plan_destroy(plan);
  zh_device_free(ctx, d_dst);
  zh_device_free(ctx, d_src);
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
  long long U;
  while (list >> name >> n_streams >> U) {
    const Case c = load(dir, name, n_streams, U);
    EXPECT(!c.rs.empty(), "%s: no ranges", name.c_str());
    run_host(ctx, c, &sum);
    run_plan(ctx, c, &sum);
    n_cases++;
  }
  EXPECT(n_cases > 0, "no cases");
  // the call errors: nothing is handed out
  uint64_t one = 1;
  size_t first[2] = {0, 0}, dl = 7;
  void* d = &one;
  int32_t st = 5;
  EXPECT(zh_uncompress_ranges(ctx, nullptr, nullptr, 0, nullptr, first, 1, &one, &one, &one, &d, &dl, &st) == ZH_ERR_ARGUMENT &&
             !d && !dl && st == ZH_OK, "ranges: a stream that is not there");
  EXPECT(zh_uncompress_ranges(ctx, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                              nullptr) == ZH_OK, "ranges: no range");
  zh_destroy(ctx);
  printf("%s: checksum %lu\n", bad ? "FAILED" : "sanitized ranges ok", sum);
  return bad ? 1 : 0;
}
