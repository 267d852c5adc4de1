// dev_mem_check.cpp -- the owners of csrc/dev_mem.hpp (DevMem, PinnedMem and their typed forms, DevBuf and its growth
// rule, TmpBufs) over stubs of the four HIP calls they name, as a program of its own so that it runs under the sanitizers.
// The stubs hand out heap blocks of exactly the size asked for (a touch past the end is the address sanitizer's),
// count what lives and record every size.  At exit nothing lives and every size is the one the caller named.
// It needs no GPU and is not part of the library; muscato_amd/build.py (CHECKS) builds it, plain and sanitized.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

namespace {
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
constexpr hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2;
hipError_t hipMalloc(void** p, size_t n) { return g_dev.get(p, n); }
hipError_t hipFree(void* p) { return g_dev.put(p); }
hipError_t hipHostMalloc(void** p, size_t n) { return g_host.get(p, n); }
hipError_t hipHostFree(void* p) { return g_host.put(p); }

#include "../dev_mem.hpp"
#include "check.hpp"

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

// ---- DevBuf

// the steps of ensure() (muscato_hip.hip) but for the keep copy: the new block first, then the old one goes
template <class T>
void grow_to(DevBuf<T>& b, uint64_t n) {
  const uint64_t ncap = grown_cap(n, b.cap);
  T* np = nullptr;
  EXPECT(hipMalloc((void**)&np, grown_bytes(ncap, sizeof(T))) == hipSuccess);
  b.release();
  b.p = np;
  b.cap = ncap;
}

void check_devbuf() {
  Heap& h = g_dev;
  const int frees0 = h.frees;
  {
    DevBuf<uint32_t> a;
    EXPECT(!a.p && a.cap == 0);
    a.release();  // of nothing
    grow_to(a, 10);
    EXPECT(a.p && a.cap == 1024 && h.live.size() == 1 && h.asked.back() == 1024 * 4 + 64);
    a.p[1023] = 7;  // the last element is the caller's
    // move: the block changes hands, nothing is freed
    DevBuf<uint32_t> b(std::move(a));
    EXPECT(!a.p && a.cap == 0 && b.cap == 1024 && b.p[1023] == 7 && h.live.size() == 1 && h.frees - frees0 == 0);
    // move-assign over a live block: that one goes, the other changes hands
    DevBuf<uint32_t> c;
    grow_to(c, 2000);
    EXPECT(c.cap == 2000 && h.live.size() == 2);
    uint32_t* const kept = b.p;
    c = std::move(b);
    EXPECT(c.p == kept && c.cap == 1024 && !b.p && b.cap == 0 && h.live.size() == 1 && h.frees - frees0 == 1);
    c = std::move(c);  // onto itself: nothing happens
    EXPECT(c.p == kept && c.cap == 1024 && h.live.size() == 1 && h.frees - frees0 == 1);
    // grown by half: one block per owner
    grow_to(c, 1025);
    EXPECT(c.cap == 1536 && h.asked.back() == 1536 * 4 + 64 && h.live.size() == 1 && h.frees - frees0 == 2);
    // release twice
    c.release();
    EXPECT(!c.p && c.cap == 0 && h.live.empty() && h.frees - frees0 == 3);
    c.release();
    EXPECT(h.frees - frees0 == 3 && h.bad_frees == 0);
    // destructor: d goes at the end of this scope
    DevBuf<uint64_t> d;
    grow_to(d, 1);
    EXPECT(d.cap == 1024 && h.asked.back() == 1024 * 8 + 64 && h.live.size() == 1);
  }
  EXPECT(h.live.empty() && h.bad_frees == 0 && h.frees - frees0 == 4);
}

// the growth rule against the lines ensure() held before grown_cap and grown_bytes
void check_growth() {
  const uint64_t V[] = {0, 1, 1023, 1024, 1025, 1ull << 20, (1ull << 32) + 1};
  for (uint64_t n : V)
    for (uint64_t cap : V) {
      uint64_t ncap = std::max<uint64_t>(n, cap + cap / 2);
      ncap = std::max<uint64_t>(ncap, 1024);
      EXPECT_MSG(grown_cap(n, cap) == ncap, "n %llu cap %llu", (unsigned long long)n, (unsigned long long)cap);
      EXPECT_MSG(grown_cap(n, cap) >= n && grown_cap(n, cap) >= 1024, "n %llu cap %llu", (unsigned long long)n, (unsigned long long)cap);
      for (uint64_t elem : {1, 2, 4, 8, 16})
        EXPECT_MSG(grown_bytes(ncap, elem) == ncap * elem + 64, "cap %llu of %llu bytes", (unsigned long long)ncap, (unsigned long long)elem);
    }
}

// ---- TmpBufs

void check_tmpbufs() {
  Heap& h = g_dev;
  {
    TmpBufs B;
    uint32_t* a = nullptr;
    char* z = nullptr;
    EXPECT(B.alloc(&a, 40) == hipSuccess && a && h.asked.back() == 40);
    a[9] = 1;
    EXPECT(B.alloc(&z, 0) == hipSuccess && z && h.asked.back() == 16);  // nothing asked for: 16 bytes
    EXPECT(B.n == 2 && h.live.size() == 2);
    B.release();
    EXPECT(B.n == 0 && h.live.empty());
    B.release();  // twice
    EXPECT(h.bad_frees == 0);
    // the 17th allocation is refused before the allocator is asked: the 16 stay held, nothing leaks
    unsigned char* q[17];
    for (int i = 0; i < 16; i++) EXPECT(B.alloc(&q[i], (size_t)i + 1) == hipSuccess && q[i]);
    const size_t asked = h.asked.size();
    q[16] = q[0];
    EXPECT(B.alloc(&q[16], 5) == hipErrorOutOfMemory && !q[16] && h.asked.size() == asked && B.n == 16 && h.live.size() == 16);
    B.release();
    EXPECT(h.live.empty() && h.bad_frees == 0);
    // an allocation that fails is not held
    h.fail_above = 100;
    EXPECT(B.alloc(&a, 101) != hipSuccess && !a && B.n == 0 && h.live.empty());
    h.fail_above = ~(size_t)0;
    // destructor: these two go at the end of this scope
    EXPECT(B.alloc(&a, 8) == hipSuccess && B.alloc(&z, 3) == hipSuccess && h.live.size() == 2);
  }
  EXPECT(h.live.empty() && h.bad_frees == 0);
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
  const size_t host_asked = g_host.asked.size();
  check_devbuf();
  check_growth();
  check_tmpbufs();
  EXPECT(g_host.asked.size() == host_asked);  // (device memory, all of it)
  EXPECT(g_dev.live.empty() && g_host.live.empty() && g_dev.bad_frees == 0 && g_host.bad_frees == 0);
  return check_done("dev_mem_check");
}
