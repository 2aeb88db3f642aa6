// bbq_mem.h - the owners of HIP memory and events in the host code: every hipMalloc / hipHostMalloc / hipEventCreate of libbbq and the
// matching release live here.  Move-only, counted in elements, no pooling and no rounding: a caller that wants headroom asks for it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace bbq {

// kPinned false: device memory (hipMalloc); true: pinned host memory (hipHostMalloc with the flags given at construction)
template <class T, bool kPinned>
class HipBuf {
 public:
  explicit HipBuf(unsigned flags = hipHostMallocDefault) : flags_(flags) {}
  HipBuf(HipBuf &&o) noexcept : p_(o.p_), n_(o.n_), flags_(o.flags_) { o.p_ = nullptr; o.n_ = 0; }
  HipBuf &operator=(HipBuf &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_; n_ = o.n_; flags_ = o.flags_;
      o.p_ = nullptr; o.n_ = 0;
    }
    return *this;
  }
  ~HipBuf() { reset(); }
  // releases what it holds and allocates exactly n elements; on failure the buffer is empty
  hipError_t alloc(size_t n) {
    reset();
    void *p = nullptr;
    const hipError_t e = kPinned ? hipHostMalloc(&p, n * sizeof(T), flags_) : hipMalloc(&p, n * sizeof(T));
    if (e != hipSuccess) return e;
    p_ = static_cast<T *>(p);
    n_ = n;
    return hipSuccess;
  }
  // grow-only: nothing happens while n elements fit
  hipError_t reserve(size_t n) { return n <= n_ ? hipSuccess : alloc(n); }
  void reset() {
    if (p_) (void)(kPinned ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr;
    n_ = 0;
  }
  T *get() const { return p_; }
  operator T *() const { return p_; }
  size_t size() const { return n_; }

 private:
  T *p_ = nullptr;
  size_t n_ = 0;
  unsigned flags_;
};
template <class T> using DevBuf = HipBuf<T, false>;
template <class T> using PinnedBuf = HipBuf<T, true>;

class Event {
 public:
  Event() = default;
  Event(Event &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  Event &operator=(Event &&o) noexcept {
    if (this != &o) {
      reset();
      e_ = o.e_;
      o.e_ = nullptr;
    }
    return *this;
  }
  ~Event() { reset(); }
  hipError_t create(unsigned flags = hipEventDefault) {
    reset();
    return hipEventCreateWithFlags(&e_, flags);
  }
  void reset() {
    if (e_) (void)hipEventDestroy(e_);
    e_ = nullptr;
  }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

}  // namespace bbq
