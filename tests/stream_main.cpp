// Stand-alone driver for zh_compress_stream_batch under -fsanitize=address,undefined (built by
// tests/test_stream_sanitize.py from zippy_amd/csrc against the emulator runtime of tests/hipemu).  Its argument is the
// directory of the file tests/stream_cases.py dumped: u32 calls; a call: u32 streams, i32 level, u32 format, u64
// block_bytes; a stream: state (u64 length, all ones: none; bytes), piece (u64, bytes), u8 flush, then what the model
// answers: i32 status, output (u64, bytes), state (as above).  Every call is made as dumped, from exact-size heap
// copies, every answer held against the model's byte for byte.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../include/zippy_hip.h"

static int bad = 0;
#define EXPECT(cond, ...)            \
  do {                               \
    if (!(cond)) {                   \
      fprintf(stderr, __VA_ARGS__);  \
      fprintf(stderr, "\n");         \
      bad++;                         \
    }                                \
  } while (0)

struct Reader {
  std::string d;
  size_t at = 0;
  template <class T>
  T get() {
    T v;
    if (at + sizeof(T) > d.size()) {
      fprintf(stderr, "the dump ends early\n");
      exit(2);
    }
    memcpy(&v, d.data() + at, sizeof(T));
    at += sizeof(T);
    return v;
  }
  bool blob(std::string& out) {  // false: none
    const uint64_t n = get<uint64_t>();
    out.clear();
    if (n == ~0ull) return false;
    if (at + n > d.size()) {
      fprintf(stderr, "the dump ends early\n");
      exit(2);
    }
    out.assign(d.data() + at, n);
    at += n;
    return true;
  }
};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  Reader r;
  {
    std::ifstream f(std::string(argv[1]) + "/cases.bin", std::ios::binary);
    r.d.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  }
  zh_ctx* ctx = nullptr;
  if (zh_create(0, nullptr, &ctx) != ZH_OK) {
    fprintf(stderr, "zh_create failed\n");
    return 2;
  }
  zh_set_gzip_fname_len(ctx, 0);
  const uint32_t ncalls = r.get<uint32_t>();
  size_t streams = 0;
  for (uint32_t c = 0; c < ncalls; c++) {
    const uint32_t n = r.get<uint32_t>();
    const int32_t level = r.get<int32_t>();
    const uint32_t fmt = r.get<uint32_t>();
    const uint64_t bb = r.get<uint64_t>();
    std::vector<std::string> state(n), data(n), want_out(n), want_state(n);
    std::vector<char> has_state(n), want_has_state(n);
    std::vector<uint8_t> flush(n);
    std::vector<int32_t> want_st(n);
    for (uint32_t i = 0; i < n; i++) {
      has_state[i] = r.blob(state[i]);
      r.blob(data[i]);
      flush[i] = r.get<uint8_t>();
      want_st[i] = r.get<int32_t>();
      r.blob(want_out[i]);
      want_has_state[i] = r.blob(want_state[i]);
    }
    // exact-size copies on the heap: a read behind a piece's or a state's end is the sanitizer's to see
    std::vector<std::vector<char>> src_mem(n), state_mem(n);
    std::vector<const void*> srcs(n), states(n);
    std::vector<size_t> lens(n), state_lens(n), dst_lens(n), nstate_lens(n);
    std::vector<void*> dsts(n), nstates(n);
    std::vector<int32_t> st(n);
    for (uint32_t i = 0; i < n; i++) {
      src_mem[i].assign(data[i].begin(), data[i].end());
      state_mem[i].assign(state[i].begin(), state[i].end());
      srcs[i] = src_mem[i].empty() ? (const void*)"" : src_mem[i].data();
      lens[i] = src_mem[i].size();
      states[i] = has_state[i] ? (state_mem[i].empty() ? (const void*)"" : state_mem[i].data()) : nullptr;
      state_lens[i] = state_mem[i].size();
    }
    const int rc = zh_compress_stream_batch(ctx, srcs.data(), lens.data(), n, level, (int)fmt, (size_t)bb, states.data(),
                                            state_lens.data(), flush.data(), dsts.data(), dst_lens.data(), nstates.data(),
                                            nstate_lens.data(), st.data());
    EXPECT(rc == ZH_OK, "call %u: %d", c, rc);
    for (uint32_t i = 0; i < n && rc == ZH_OK; i++) {
      streams++;
      EXPECT(st[i] == want_st[i], "call %u stream %u: status %d, want %d", c, i, st[i], want_st[i]);
      if (st[i] != ZH_OK || want_st[i] != ZH_OK) {
        EXPECT(!dsts[i] && !nstates[i], "call %u stream %u: a failed stream has results", c, i);
      } else {
        EXPECT(dst_lens[i] == want_out[i].size() && (!dst_lens[i] || !memcmp(dsts[i], want_out[i].data(), dst_lens[i])),
               "call %u stream %u: output (%zu bytes, want %zu)", c, i, dst_lens[i], want_out[i].size());
        EXPECT((nstates[i] != nullptr) == (bool)want_has_state[i] && nstate_lens[i] == want_state[i].size() &&
                   (!nstate_lens[i] || !memcmp(nstates[i], want_state[i].data(), nstate_lens[i])),
               "call %u stream %u: state", c, i);
      }
      zh_free(dsts[i]);
      zh_free(nstates[i]);
    }
  }
  zh_destroy(ctx);
  if (bad) return 1;
  printf("sanitized stream ok: %u calls, %zu streams\n", ncalls, streams);
  return 0;
}
