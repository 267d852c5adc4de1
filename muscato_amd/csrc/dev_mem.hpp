// dev_mem.hpp -- the owners of device memory and of pinned host memory.  OwnedMem: one block of exactly the size asked
// for, freed when its owner goes.  DevBuf: a work buffer of the passes, grown by half (grown_cap, grown_bytes).  TmpBufs:
// the temporary blocks of one call.  All move-only or fixed in place.  This header includes no HIP header and names
// hipMalloc / hipFree / hipHostMalloc / hipHostFree (and hipError_t, hipSuccess, hipErrorOutOfMemory) unqualified:
// muscato_hip.hip includes it after <hip/hip_runtime.h>, host/dev_mem_check.cpp after stubs of its own that count what lives.
#pragma once

#include <cstddef>
#include <cstdint>
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
