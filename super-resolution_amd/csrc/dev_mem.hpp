// dev_mem.hpp -- the only place of libsrmap.so that allocates device or pinned host memory: two move-only owners and
// the count of the blocks they hold (srmap_live_allocations, a leak diagnostic).  An owner frees with a plain
// hipFree / hipHostFree when it is reset or goes out of scope: work in flight that reads the block must have been
// waited for by then, exactly as before a hand-written free.  An owner is NEVER a member of a struct passed to a
// kernel by value (the argument is copied bytewise; the host copy's destructor would free live memory): kernels take
// raw pointers, obtained with as<T>() at the launch site.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>

namespace srmap {

inline std::atomic<long long> g_live_allocations{0};

// One hipMalloc block, or nothing.
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
    return *this;
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }
  // frees what it held, then allocates (0 bytes: 8).  On failure it holds nothing and HIP's last-error word is cleared
  hipError_t alloc(size_t bytes) {
    reset();
    const hipError_t e = hipMalloc(&p_, bytes ? bytes : 8);
    if (e == hipSuccess) { ++g_live_allocations; } else { p_ = nullptr; (void)hipGetLastError(); }
    return e;
  }
  void reset() {
    if (p_) { (void)hipFree(p_); --g_live_allocations; }
    p_ = nullptr;
  }
  // gives the block away without freeing it: it is the caller's from here on (and no longer counted)
  void* release() {
    if (p_) --g_live_allocations;
    void* q = p_;
    p_ = nullptr;
    return q;
  }
  template <typename T = void>
  T* as() const { return static_cast<T*>(p_); }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  void* p_ = nullptr;
};

// The same over hipHostMalloc(bytes, flags) / hipHostFree.
class PinnedBuf {
 public:
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
    return *this;
  }
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { reset(); }
  hipError_t alloc(size_t bytes, unsigned flags = hipHostMallocDefault) {
    reset();
    const hipError_t e = hipHostMalloc(&p_, bytes ? bytes : 8, flags);
    if (e == hipSuccess) { ++g_live_allocations; } else { p_ = nullptr; (void)hipGetLastError(); }
    return e;
  }
  void reset() {
    if (p_) { (void)hipHostFree(p_); --g_live_allocations; }
    p_ = nullptr;
  }
  void* release() {
    if (p_) --g_live_allocations;
    void* q = p_;
    p_ = nullptr;
    return q;
  }
  template <typename T = void>
  T* as() const { return static_cast<T*>(p_); }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  void* p_ = nullptr;
};

}  // namespace srmap
