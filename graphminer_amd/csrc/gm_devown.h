// gm_devown.h -- DevOwn<T>: the one owner of a PERSISTENT device array (a member of a handle, a table, a plan).
// A struct that holds device memory says so by the type of the member; it needs no destructor, no free list and no "owned" flag, and a
// setup function that fails half way gives back what it built when its locals go out of scope.  A borrowed array stays a plain T *.
// Move-only; no sharing, no reference count, no deleter other than dev_free.  (DevBuf, gm_host.h, is the other kind: the pooled or cached
// temporary of a setup scope.)  Needs nothing but hipError_t and the library's allocator, so a plain host compiler builds it.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>

hipError_t dev_malloc_bytes(void **p, size_t bytes);  // gm_graph.hip
void dev_free(void *p);

template <class T>
class DevOwn {
  T *p_ = nullptr;

 public:
  DevOwn() = default;
  DevOwn(const DevOwn &) = delete;
  DevOwn &operator=(const DevOwn &) = delete;
  DevOwn(DevOwn &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevOwn &operator=(DevOwn &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_;
      o.p_ = nullptr;
    }
    return *this;
  }
  ~DevOwn() { reset(); }
  void reset() {
    if (p_) dev_free(p_);
    p_ = nullptr;
  }
  // `bytes` of fresh device memory; what it held before goes back first.  On an error it is left empty.
  hipError_t alloc(size_t bytes) {
    reset();
    void *q = nullptr;
    const hipError_t e = dev_malloc_bytes(&q, bytes);
    if (e == hipSuccess) p_ = static_cast<T *>(q);
    return e;
  }
  // takes over the array of a DevBuf<T> that was allocated with keep = true (a pooled one hands over nothing)
  template <class Buf>
  void take(Buf &b) {
    reset();
    p_ = b.release();
  }
  T *get() const { return p_; }
  operator T *() const { return p_; }  // kernel arguments, `g->d_rp + v`, `if (!g->d_x)`, `p.rp = g->d_rp` read as with a raw pointer
};
