// dev_mem_check.cpp -- the owners of csrc/dev_mem.hpp (DevMem, PinnedMem and their typed forms, DevBuf and its growth
// rule, TmpBufs, Readback) over stubs of the six HIP calls they name, as a program of its own so that it runs under the
// sanitizers.  The stubs hand out heap blocks of exactly the size asked for (a touch past the end is the address
// sanitizer's), count what lives and record every size.  At exit nothing lives and every size is the one the caller named.
// A stubbed copy is deferred: recorded when it is queued and performed by the stubbed stream wait only, so that a copy
// whose destination has gone by then is the address sanitizer's too.
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

struct Copy {
  void* dst;
  const void* src;
  size_t n;
};
struct Stream {
  std::vector<Copy> pending;
  int queued = 0, waits = 0;
  int fail_copy = -1;  // the copy with this number (of all queued so far) is refused
  bool fail_wait = false;
} g_stream;

typedef int hipError_t;
typedef Stream* hipStream_t;
constexpr hipError_t hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2, hipErrorStub = 77, hipErrorStubWait = 78;
enum hipMemcpyKind { hipMemcpyDeviceToHost = 2 };
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind, hipStream_t st) {
  if (st->queued++ == st->fail_copy) return hipErrorStub;
  st->pending.push_back(Copy{dst, src, n});
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t st) {
  st->waits++;
  for (const Copy& k : st->pending) memcpy(k.dst, k.src, k.n);  // (performed even when the wait reports an error)
  st->pending.clear();
  return st->fail_wait ? hipErrorStubWait : hipSuccess;
}
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

// ---- Readback

void check_readback() {
  Stream& S = g_stream;
  uint64_t words[4];
  memset(words, 0xEE, sizeof words);
  PinnedWords P;
  P.w = words;
  P.n = 4;
  const uint64_t d64 = 0x1122334455667788ull, dpair[2] = {7, ~0ull};
  const uint32_t d32 = 0xA1B2C3D4u;
  const unsigned char d8 = '\n';
  // the words are handed out in order, each zeroed first; a 1-byte and a 4-byte read arrive zero-extended; nothing
  // reaches a destination before wait()
  {
    Readback R(P, &S);
    uint64_t a = 1, b = 2, c = 3;
    unsigned char e = 4;
    R.get(&d64, &a);
    R.get(&d32, &b);
    R.get(&d8, &c);
    R.get(&d8, &e);
    EXPECT(S.pending.size() == 4 && P.holder == &R);
    for (size_t i = 0; i < S.pending.size(); i++) EXPECT(S.pending[i].dst == words + i);
    EXPECT(S.pending[0].n == 8 && S.pending[1].n == 4 && S.pending[2].n == 1 && S.pending[3].n == 1);
    EXPECT(words[0] == 0 && words[1] == 0 && words[2] == 0 && words[3] == 0);
    EXPECT(a == 1 && b == 2 && c == 3 && e == 4 && S.waits == 0);
    EXPECT(R.wait() == hipSuccess && S.waits == 1 && S.pending.empty() && !P.holder);
    EXPECT(a == d64 && b == d32 && c == d8 && e == d8);
    // the object serves again, from the first word
    uint32_t f = 9;
    R.get(&d32, &f);
    EXPECT(S.pending.size() == 1 && S.pending[0].dst == words && f == 9);
    EXPECT(R.wait() == hipSuccess && f == d32 && S.waits == 2);
  }
  EXPECT(S.waits == 2);  // (nothing was queued when it went)
  // a read of consecutive 64-bit words beside a scalar
  {
    Readback R(P, &S);
    uint64_t two[2] = {1, 1};
    uint32_t x = 0;
    R.get(&d32, &x);
    R.get_words(dpair, two, 2);
    EXPECT(S.pending.size() == 2 && S.pending[1].dst == words + 1 && S.pending[1].n == 16 && two[0] == 1);
    EXPECT(R.wait() == hipSuccess && two[0] == 7 && two[1] == ~0ull && x == d32);
  }
  // one request too many is an error of wait(), and nothing is written: not past the block, not to any destination
  {
    Readback R(P, &S);
    uint64_t v[5] = {10, 11, 12, 13, 14}, two[2] = {5, 5};
    const uint64_t guard = words[3];
    for (int i = 0; i < 3; i++) R.get(&d64, &v[i]);
    R.get_words(dpair, two, 2);  // two words where one is left
    R.get(&d64, &v[3]);          // (refused as well: the first error stands)
    EXPECT(S.pending.size() == 3 && words[3] == guard);
    EXPECT(R.wait() == hipErrorInvalidValue && S.pending.empty() && !P.holder);
    EXPECT(v[0] == 10 && v[1] == 11 && v[2] == 12 && v[3] == 13 && two[0] == 5 && two[1] == 5);
    EXPECT(R.wait() == hipSuccess);  // (the error was that wait's)
  }
  // the first queueing error wins, over later ones and over the wait's; the wait still happens; no destination is touched
  {
    Readback R(P, &S);
    uint64_t a = 1, b = 2, c = 3;
    const int waits = S.waits;
    R.get(&d64, &a);
    S.fail_copy = S.queued;
    R.get(&d64, &b);
    S.fail_copy = -1;
    R.get(&d64, &c);
    R.get_words(dpair, &c, 9);
    S.fail_wait = true;
    EXPECT(R.wait() == hipErrorStub && S.waits == waits + 1 && S.pending.empty());
    EXPECT(a == 1 && b == 2 && c == 3);
    // a failed wait alone: its error, and again nothing is delivered
    R.get(&d64, &a);
    EXPECT(R.wait() == hipErrorStubWait && a == 1);
    S.fail_wait = false;
    R.get(&d64, &a);
    EXPECT(R.wait() == hipSuccess && a == d64);
  }
  // an object dropped without wait() has waited, nothing of it is pending afterwards and nothing was delivered -- the
  // destination may be gone by then (a frame that returned early): the deferred copy never aimed at it
  {
    const int waits = S.waits;
    uint64_t* gone = new uint64_t(5);
    uint64_t kept = 6;
    {
      Readback R(P, &S);
      R.get(&d64, gone);
      R.get(&d64, &kept);
      delete gone;
      EXPECT(S.pending.size() == 2);
    }
    EXPECT(S.waits == waits + 1 && S.pending.empty() && !P.holder && kept == 6);
  }
  // while one Readback has copies queued, another is refused the words (no two helpers on the same word)
  {
    Readback R(P, &S), Q(P, &S);
    uint64_t a = 1, b = 2;
    R.get(&d64, &a);
    Q.get(&d32, &b);
    EXPECT(S.pending.size() == 1 && Q.wait() == hipErrorInvalidValue && b == 2 && P.holder == &R);
    EXPECT(R.wait() == hipSuccess && a == d64);
    Q.get(&d32, &b);  // (free again)
    EXPECT(Q.wait() == hipSuccess && b == d32);
  }
  EXPECT(S.pending.empty() && !P.holder);
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
  check_readback();
  EXPECT(g_host.asked.size() == host_asked);  // (device memory, all of it)
  EXPECT(g_dev.live.empty() && g_host.live.empty() && g_dev.bad_frees == 0 && g_host.bad_frees == 0);
  return check_done("dev_mem_check");
}
