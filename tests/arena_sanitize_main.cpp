// Stand-alone driver for the typed arena of zippy_amd/csrc/zh_host.h under -fsanitize=address,undefined (built by
// tests/test_arena_sanitize.py against the emulator runtime of tests/hipemu, where device memory is host memory):
// arrays of five element types and of 0, 1, 63, 64 and 65 elements, with and without a host source, bound to const and
// non-const pointers.  Offsets and the total are held against the byte-counting reserve() the arena replaced.
#include <stdio.h>

#include <functional>
#include <list>
#include <vector>

#include "../zippy_amd/csrc/zh_host.h"

struct S24 {
  uint64_t a, b, c;
};
static_assert(sizeof(S24) == 24, "a 24-byte element");

struct OldArena {  // what every site spelled by hand: bytes in, offset out
  size_t size = 0;
  size_t reserve(size_t bytes) {
    size_t off = (size + 255) & ~(size_t)255;
    size = off + bytes;
    return off;
  }
};

struct Want {
  std::function<const void*()> bound;  // the pointer the arena was given
  size_t off, bytes;
  const void* src;
};

static int bad = 0;
#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      fprintf(stderr, "line %d: %s\n", __LINE__, #cond);          \
      bad++;                                                      \
    }                                                             \
  } while (0)

template <class T>
struct Array {
  T* p = nullptr;
  const T* cp = nullptr;
  std::vector<T> src;
};

// One array of `count` elements: every other one with a source, every third bound to a pointer to const
template <class T>
static void declare(Arena& ar, OldArena& old, std::list<Array<T>>& keep, std::vector<Want>& want, size_t count) {
  const size_t k = want.size();
  keep.emplace_back();
  Array<T>& a = keep.back();  // (a list: the registered pointers stay where they are)
  const bool with_src = k % 2 == 0, to_const = k % 3 == 0;
  if (with_src) {
    a.src.resize(count);
    unsigned char* bytes = reinterpret_cast<unsigned char*>(a.src.data());
    for (size_t i = 0; i < count * sizeof(T); i++) bytes[i] = (unsigned char)(31 * k + 7 * i + 1);
  }
  const T* src = with_src ? a.src.data() : nullptr;
  if (to_const) {
    if (with_src) ar.add(a.cp, count, src); else ar.add(a.cp, count);
    want.push_back(Want{[&a] { return (const void*)a.cp; }, old.reserve(count * sizeof(T)), count * sizeof(T), src});
  } else {
    if (with_src) ar.add(a.p, count, src); else ar.add(a.p, count);
    want.push_back(Want{[&a] { return (const void*)a.p; }, old.reserve(count * sizeof(T)), count * sizeof(T), src});
  }
}

int main() {
  zh_ctx* ctx = nullptr;
  if (zh_create(0, nullptr, &ctx)) return 3;
  {
    Arena ar;
    OldArena old;
    std::list<Array<uint8_t>> a8;
    std::list<Array<uint16_t>> a16;
    std::list<Array<uint32_t>> a32;
    std::list<Array<uint64_t>> a64;
    std::list<Array<S24>> a24;
    std::vector<Want> want;
    const size_t counts[5] = {0, 1, 63, 64, 65};
    for (int round = 0; round < 2; round++)  // (twice: every type meets a source and a const pointer at some count)
      for (size_t c = 0; c < 5; c++) {
        const size_t count = counts[(c + round) % 5];
        declare(ar, old, a8, want, count);
        declare(ar, old, a16, want, count);
        declare(ar, old, a32, want, count);
        declare(ar, old, a64, want, count);
        declare(ar, old, a24, want, count);
      }
    declare(ar, old, a32, want, 0);  // an empty array last: its pointer is the end
    CHECK(ar.size == old.size);
    const size_t arrays_end = ar.size;
    CHECK(ar.pad(256) == old.reserve(256));  // the tail the sites keep behind the last array
    CHECK(ar.size == old.size && ar.size == ((arrays_end + 255) & ~(size_t)255) + 256);
    DevBuf mem;
    CHECK(ar.alloc(ctx, mem) == hipSuccess && mem.p && ar.base == mem.p);
    memset(mem.p, 0xEE, ar.size);
    ar.bind();
    size_t running = 0;
    for (size_t k = 0; k < want.size(); k++) {
      const Want& w = want[k];
      const unsigned char* p = (const unsigned char*)w.bound();
      running = (running + 255) & ~(size_t)255;
      CHECK(w.off % 256 == 0 && w.off == running);
      running += w.bytes;
      CHECK(p != nullptr && p == mem.p + w.off);
      if (!w.bytes) CHECK(p == (k + 1 < want.size() ? mem.p + want[k + 1].off : mem.p + arrays_end));
    }
    CHECK(running == arrays_end);
    CHECK(ar.upload(ctx->stream) == hipSuccess);
    std::vector<unsigned char> image(arrays_end, 0xEE);
    ar.gather(image.data());
    for (const Want& w : want) {
      const unsigned char* p = (const unsigned char*)w.bound();
      if (w.src) {
        CHECK(memcmp(p, w.src, w.bytes) == 0);
        CHECK(memcmp(image.data() + w.off, w.src, w.bytes) == 0);
      } else {
        for (size_t i = 0; i < w.bytes; i++) CHECK(p[i] == 0xEE);  // (not uploaded: untouched)
      }
    }
    // a host copy of the arena, and an array of it by its device pointer
    const Array<uint64_t>& some = a64.back();
    const uint64_t* dev = some.p ? some.p : some.cp;
    CHECK((const unsigned char*)ar.host(image.data(), dev) == image.data() + ((const unsigned char*)dev - mem.p));
    // clear() zeroes one array by its declaration and nothing else
    Array<S24>& z = *std::next(a24.begin(), 4);  // (the one of 65 elements)
    const size_t zb = (z.p ? (unsigned char*)z.p : (unsigned char*)z.cp) - mem.p;
    CHECK((z.p ? ar.clear(z.p, ctx->stream) : ar.clear(z.cp, ctx->stream)) == hipSuccess);
    size_t zbytes = 0;
    for (const Want& w : want)
      if (w.off == zb && w.bytes) zbytes = w.bytes;
    CHECK(zbytes != 0);
    for (size_t i = 0; i < zbytes; i++) CHECK(mem.p[zb + i] == 0);
    CHECK(mem.p[zb + zbytes] == 0xEE);
    uint32_t* stranger = nullptr;
    CHECK(ar.clear(stranger, ctx->stream) != hipSuccess);
  }
  {  // nothing declared: allocates and binds, and touches nothing
    Arena none;
    DevBuf mem;
    CHECK(none.alloc(ctx, mem) == hipSuccess && mem.p != nullptr && none.size == 0);
    none.bind();
    CHECK(none.upload(ctx->stream) == hipSuccess);
    none.gather(nullptr);
  }
  zh_destroy(ctx);
  printf("%s\n", bad ? "FAILED" : "sanitized arena ok");
  return bad ? 1 : 0;
}
