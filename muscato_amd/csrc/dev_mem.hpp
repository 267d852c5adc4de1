// dev_mem.hpp -- the owners of device memory and of pinned host memory: one block of exactly the size asked for, freed
// when its owner goes.  Move-only.  This header includes no HIP header and names hipMalloc / hipFree / hipHostMalloc /
// hipHostFree (and hipError_t, hipSuccess) unqualified: muscato_hip.hip includes it after <hip/hip_runtime.h>,
// host/dev_mem_check.cpp after stubs of its own that count what lives.
#pragma once

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
