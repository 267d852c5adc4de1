// dev_mem.hpp -- the owners of device memory and of pinned host memory.  OwnedMem: one block of exactly the size asked
// for, freed when its owner goes.  DevBuf: a work buffer of the passes, grown by half (grown_cap, grown_bytes).  TmpBufs:
// the temporary blocks of one call.  Readback: scalars on their way from the device to the host, through the pinned words
// of a context, with one wait.  All move-only or fixed in place.  This header includes no HIP header and names
// hipMalloc / hipFree / hipHostMalloc / hipHostFree / hipMemcpyAsync / hipStreamSynchronize (and hipError_t, hipStream_t,
// hipSuccess, hipErrorOutOfMemory, hipErrorInvalidValue, hipMemcpyDeviceToHost) unqualified: muscato_hip.hip includes it
// after <hip/hip_runtime.h>, host/dev_mem_check.cpp after stubs of its own that count what lives and defer every copy.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <utility>

template <class Api>
struct OwnedMem {
  void* p = nullptr;
  uint64_t bytes = 0;
  OwnedMem() = default;  // (the moves below delete the copies)
  OwnedMem(OwnedMem&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
  OwnedMem& operator=(OwnedMem&& o) noexcept {
    if (this != &o) release(), p = std::exchange(o.p, nullptr), bytes = std::exchange(o.bytes, 0);
    return *this;
  }
  ~OwnedMem() { release(); }
  // a new block of n bytes in place of the one held (which goes first)
  hipError_t alloc(uint64_t n) {
    release();
    const hipError_t e = Api::get(&p, n);
    if (e == hipSuccess) bytes = n; else p = nullptr;
    return e;
  }
  // a table that is grown to what is asked for and never shrunk (hipMalloc / hipFree of tens of GiB take seconds)
  hipError_t grow(uint64_t n) { return p && bytes >= n ? hipSuccess : alloc(n); }
  void release() {
    if (p) (void)Api::put(p);
    p = nullptr;
    bytes = 0;
  }
};

struct DeviceApi {
  static hipError_t get(void** p, uint64_t n) { return hipMalloc(p, n); }
  static hipError_t put(void* p) { return hipFree(p); }
};
struct PinnedApi {
  static hipError_t get(void** p, uint64_t n) { return hipHostMalloc(p, n); }
  static hipError_t put(void* p) { return hipHostFree(p); }
};
typedef OwnedMem<DeviceApi> DevMem;
typedef OwnedMem<PinnedApi> PinnedMem;

// a block read as an array of T: stands where a T* stood
template <class T, class Mem = DevMem>
struct Typed : Mem {
  T* get() const { return static_cast<T*>(this->p); }
  operator T*() const { return get(); }
};
template <class T> using DevPtr = Typed<T, DevMem>;
template <class T> using PinnedPtr = Typed<T, PinnedMem>;

// a work buffer of the passes: grown by half when it is too small (ensure, muscato_hip.hip), freed with its owner.
// A sibling of Typed<T>, not one: the kernel launches read its p as a T*, and ensure() takes the new block before the
// old one goes (the keep copy reads it), where OwnedMem::alloc releases first.
template <class T>
struct DevBuf {
  T* p = nullptr;
  uint64_t cap = 0;  // elements
  DevBuf() = default;  // (move-only: the moves delete the copies)
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) release(), p = std::exchange(o.p, nullptr), cap = std::exchange(o.cap, 0);
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// the growth rule of ensure(): the elements a buffer of cap holds after it is asked for n (n > cap, or nothing is held) --
// what is asked for or half as much again as before, whichever is more, and never fewer than 1024 ...
inline uint64_t grown_cap(uint64_t n, uint64_t cap) {
  const uint64_t by_half = cap + cap / 2, want = n > by_half ? n : by_half;
  return want > 1024 ? want : 1024;
}
// ... and the bytes asked of hipMalloc for them: 64 of slack behind the last element
inline uint64_t grown_bytes(uint64_t cap, uint64_t elem_bytes) { return cap * elem_bytes + 64; }

// temporary device allocations of one call, released on every exit path
struct TmpBufs {
  void* p[16] = {};
  int n = 0;
  template <class T>
  hipError_t alloc(T** out, size_t bytes) {
    void* q = nullptr;
    *out = nullptr;
    if (n >= 16) return hipErrorOutOfMemory;  // (more allocations than this helper was sized for)
    const hipError_t e = hipMalloc(&q, bytes ? bytes : 16);
    if (e == hipSuccess) p[n++] = q;
    *out = (T*)q;
    return e;
  }
  void release() {
    for (int i = 0; i < n; i++) (void)hipFree(p[i]);
    n = 0;
  }
  ~TmpBufs() { release(); }
};

// The pinned words scalars come back through (musc_ctx::h_pinned), and the Readback that has copies queued into them.
struct PinnedWords {
  uint64_t* w = nullptr;
  unsigned n = 0;
  const void* holder = nullptr;
};

// Scalars read back from the device, for one wait: get() queues a copy of a device value into the next free pinned
// word, zeroed first, and notes where it belongs; wait() waits for the stream once and then hands every word to its
// destination, zero-extended to the destination's width.  A destination may be a local variable: no copy ever aims at
// it, and nothing is written to it before a wait() that succeeded.  wait() returns the first error of any get(), else
// the wait's own.  One request too many, or a get() while another Readback holds the words, is such an error and never
// a write.  An object that goes with copies queued waits for the stream and delivers nothing.
class Readback {
 public:
  static constexpr unsigned MAX_WORDS = 16;
  Readback(PinnedWords& words, hipStream_t stream) : P(words), st(stream) {}
  Readback(const Readback&) = delete;  // (nor assigned: P is a reference)
  ~Readback() { if (P.holder == this) (void)wait_only(); }
  // *dst = *src, once wait() has returned hipSuccess
  template <class S, class T>
  Readback& get(const S* src, T* dst) {
    static_assert(std::is_integral<S>::value && std::is_integral<T>::value && sizeof(S) <= sizeof(T) && sizeof(T) <= 8, "a scalar into one as wide or wider");
    return queue(src, sizeof(S), 1, dst, sizeof(T));
  }
  // dst[0 .. nwords) = src[0 .. nwords), consecutive 64-bit words
  template <class S>
  Readback& get_words(const S* src, uint64_t* dst, unsigned nwords) {
    static_assert(std::is_integral<S>::value && sizeof(S) == 8, "64-bit words");
    return queue(src, 8 * nwords, nwords, dst, 8 * nwords);
  }
  hipError_t wait() {
    const hipError_t es = wait_only(), e = err != hipSuccess ? err : es;
    if (e == hipSuccess)
      for (unsigned i = 0; i < nd; i++) memcpy(q[i].dst, P.w + q[i].word, q[i].bytes);
    nd = 0, err = hipSuccess;
    return e;
  }

 private:
  struct Dest { void* dst; unsigned word, bytes; };
  Readback& queue(const void* src, unsigned src_bytes, unsigned nwords, void* dst, unsigned dst_bytes) {
    if (err != hipSuccess) return *this;
    if ((P.holder && P.holder != this) || nwords > P.n - nq || nwords > MAX_WORDS - nq) return err = hipErrorInvalidValue, *this;
    P.holder = this;
    memset(P.w + nq, 0, 8 * nwords);
    if ((err = hipMemcpyAsync(P.w + nq, src, src_bytes, hipMemcpyDeviceToHost, st)) != hipSuccess) return *this;
    q[nd++] = Dest{dst, nq, dst_bytes};
    nq += nwords;
    return *this;
  }
  hipError_t wait_only() {
    const hipError_t e = hipStreamSynchronize(st);
    if (P.holder == this) P.holder = nullptr;
    nq = 0;
    return e;
  }
  PinnedWords& P;
  hipStream_t st;
  hipError_t err = hipSuccess;
  Dest q[MAX_WORDS];
  unsigned nq = 0, nd = 0;  // words taken; destinations noted
};
