// dev_mem_check.cpp -- the owners of csrc/dev_mem.hpp (DevMem, PinnedMem and their typed forms) over stubs of the four
// HIP calls they name, as a program of its own so that it runs under the sanitizers:
//     g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o dev_mem_check dev_mem_check.cpp
//     ./dev_mem_check
// The stubs hand out heap blocks of exactly the size asked for (a touch past the end is the address sanitizer's),
// count what lives and record every size.  At exit nothing lives and every size is the one the caller named.
// It needs no GPU and is not part of the library build.  Exit status 0 and "ok" on success.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

namespace {
int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      failures++;                                                 \
    }                                                             \
  } while (0)

struct Heap {
  std::map<void*, size_t> live;
  std::vector<size_t> asked;
  size_t fail_above = ~(size_t)0;  // a request larger than this fails
  int frees = 0, bad_frees = 0;
  int get(void** p, size_t n) {
    asked.push_back(n);
    if (n > fail_above) return 2;
    *p = malloc(n ? n : 1);
    live[*p] = n;
    return 0;
  }
  int put(void* p) {
    if (!live.count(p)) return bad_frees++, 1;
    live.erase(p);
    free(p);
    frees++;
    return 0;
  }
} g_dev, g_host;
}  // namespace

typedef int hipError_t;
constexpr hipError_t hipSuccess = 0;
hipError_t hipMalloc(void** p, size_t n) { return g_dev.get(p, n); }
hipError_t hipFree(void* p) { return g_dev.put(p); }
hipError_t hipHostMalloc(void** p, size_t n) { return g_host.get(p, n); }
hipError_t hipHostFree(void* p) { return g_host.put(p); }

#include "../dev_mem.hpp"

namespace {

template <class Mem>
void check(Heap& h) {
  const size_t asked0 = h.asked.size();
  const int frees0 = h.frees;
  std::vector<size_t> want;
  auto alloc = [&](Mem& m, uint64_t n) {
    want.push_back(n);
    return m.alloc(n);
  };
  {
    Mem a;
    EXPECT(!a.p && a.bytes == 0);
    a.release();  // of nothing
    EXPECT(alloc(a, 100) == hipSuccess && a.p && a.bytes == 100 && h.live.size() == 1);
    memset(a.p, 0xAB, 100);  // the whole block is the caller's
    // move: the block changes hands, nothing is freed
    Mem b(std::move(a));
    EXPECT(!a.p && a.bytes == 0 && b.bytes == 100 && h.live.size() == 1 && h.frees - frees0 == 0);
    // move-assign over a live block: that one goes, the other changes hands
    Mem c;
    EXPECT(alloc(c, 7) == hipSuccess && h.live.size() == 2);
    void* const kept = b.p;
    c = std::move(b);
    EXPECT(c.p == kept && c.bytes == 100 && !b.p && h.live.size() == 1 && h.frees - frees0 == 1);
    c = std::move(c);  // onto itself: nothing happens
    EXPECT(c.p == kept && h.live.size() == 1);
    // alloc over a live block frees it first: one block per owner, of the size last asked for
    EXPECT(alloc(c, 33) == hipSuccess && c.bytes == 33 && h.live.size() == 1 && h.frees - frees0 == 2);
    // release twice
    c.release();
    EXPECT(!c.p && c.bytes == 0 && h.live.empty() && h.frees - frees0 == 3);
    c.release();
    EXPECT(h.frees - frees0 == 3 && h.bad_frees == 0);
    // grow-if-smaller: kept when it suffices, replaced at the exact size when it does not, never shrunk
    Mem t;
    want.push_back(64);
    EXPECT(t.grow(64) == hipSuccess && t.bytes == 64);
    void* const first = t.p;
    EXPECT(t.grow(64) == hipSuccess && t.grow(1) == hipSuccess && t.p == first && t.bytes == 64);
    want.push_back(65);
    EXPECT(t.grow(65) == hipSuccess && t.bytes == 65 && h.live.size() == 1);
    // an allocation that fails leaves an empty owner (the old block went first)
    h.fail_above = 1000;
    EXPECT(alloc(t, 5000) != hipSuccess && !t.p && t.bytes == 0 && h.live.empty());
    h.fail_above = ~(size_t)0;
    // zero bytes is a block too
    EXPECT(alloc(t, 0) == hipSuccess && t.p && t.bytes == 0 && h.live.size() == 1);
    // destructor: d and t go at the end of this scope
    Mem d;
    EXPECT(alloc(d, 12) == hipSuccess && h.live.size() == 2);
  }
  EXPECT(h.live.empty() && h.bad_frees == 0);
  // every size that reached the allocator is the size the caller named: no rounding, no slack
  EXPECT(h.asked.size() - asked0 == want.size());
  for (size_t i = 0; i < want.size() && asked0 + i < h.asked.size(); i++) EXPECT(h.asked[asked0 + i] == want[i]);
}

struct Holder {  // as musc_ctx holds them: members, freed with the object
  DevPtr<uint32_t> rd;
  DevPtr<char> text;
  PinnedPtr<uint64_t> pinned;
};

}  // namespace

int main() {
  check<DevMem>(g_dev);
  EXPECT(g_host.asked.empty());  // (a device owner never touches the pinned pair)
  check<PinnedMem>(g_host);
  check<DevPtr<uint32_t>>(g_dev);
  check<PinnedPtr<uint64_t>>(g_host);
  {
    Holder* h = new Holder();
    EXPECT(h->rd.alloc(10 * 4) == hipSuccess && h->text.alloc(3) == hipSuccess && h->pinned.alloc(2 * 8) == hipSuccess);
    uint32_t* rd = h->rd;  // stands where a pointer stood
    rd[9] = 1;
    EXPECT(h->rd[9] == 1 && h->rd + 9 == rd + 9 && h->rd != nullptr && !!h->rd);
    const uint32_t* plane = g_dev.frees ? h->rd : (const uint32_t*)nullptr;
    EXPECT(plane == rd);
    h->pinned[1] = 5;
    EXPECT(*(h->pinned + 1) == 5 && h->pinned.get() == static_cast<uint64_t*>(h->pinned.p));
    EXPECT(g_dev.live.size() == 2 && g_host.live.size() == 1);
    delete h;
  }
  EXPECT(g_dev.live.empty() && g_host.live.empty() && g_dev.bad_frees == 0 && g_host.bad_frees == 0);
  if (failures) {
    fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  puts("ok");
  return 0;
}
