// dev_buf.h — the one owner of device memory: every state object of the library keeps its allocations in DevBuf members, so
// destroying the object frees them and nothing names them a second time.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>

namespace pnvo {

// Bytes held through DevBuf, device and host-mapped together (pnvo_device_bytes_live).  Handles of different host threads allocate
// concurrently.
inline std::atomic<long long> g_device_bytes_live{0};

// One allocation of `size()` elements.  Move-only; converts to T* so kernel-argument code reads as with a raw pointer.
template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p_(o.p_), n_(o.n_), host_(o.host_) { o.p_ = nullptr, o.n_ = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, n_ = o.n_, host_ = o.host_;
      o.p_ = nullptr, o.n_ = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }

  operator T *() const { return p_; }
  size_t size() const { return n_; }

  void reset() {
    if (p_) {
      (void)(host_ ? hipHostFree(p_) : hipFree(p_));
      g_device_bytes_live -= (long long)bytes(n_);
    }
    p_ = nullptr, n_ = 0;
  }
  // n elements of device memory (never fewer than 16 bytes), contents undefined; the old allocation goes first
  hipError_t alloc(size_t n) { return take(n, false, 0); }
  // n elements of host memory mapped into the device's address space (hipHostMalloc flags as given): flags both sides poll
  hipError_t alloc_host(size_t n, unsigned flags) { return take(n, true, flags); }
  // grow only
  hipError_t reserve(size_t n) { return n > n_ ? alloc(n) : hipSuccess; }
  // Synchronous host -> device copy.  Same-sized data is rewritten in place: device addresses kept elsewhere (the training step's
  // re-pack maps, captured graphs) stay valid across reloads.
  hipError_t upload(const T *src, size_t n) {
    if (!p_ || n != n_)
      if (hipError_t e = alloc(n)) return e;
    return hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice);
  }

 private:
  static size_t bytes(size_t n) { return n * sizeof(T) < 16 ? 16 : n * sizeof(T); }
  hipError_t take(size_t n, bool host, unsigned flags) {
    reset();
    void *q = nullptr;
    if (hipError_t e = host ? hipHostMalloc(&q, bytes(n), flags) : hipMalloc(&q, bytes(n))) return e;
    p_ = static_cast<T *>(q), n_ = n, host_ = host;
    g_device_bytes_live += (long long)bytes(n);
    return hipSuccess;
  }
  T *p_ = nullptr;
  size_t n_ = 0;
  bool host_ = false;
};

// Two buffers handed on as one `T *const *` (the scale / shift pair of a GroupNorm).
template <class T>
class DevPair {
 public:
  hipError_t alloc(int k, size_t n) {
    hipError_t e = buf_[k].alloc(n);
    view_[k] = buf_[k];
    return e;
  }
  void reset() {
    for (int k = 0; k < 2; ++k) buf_[k].reset(), view_[k] = nullptr;
  }
  T *operator[](int k) const { return view_[k]; }
  operator T *const *() const { return view_; }

 private:
  DevBuf<T> buf_[2];
  T *view_[2] = {nullptr, nullptr};
};

}  // namespace pnvo
