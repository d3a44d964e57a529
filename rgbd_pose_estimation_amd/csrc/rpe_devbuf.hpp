// The one place in the host units that allocates and frees plain device memory (pinned host memory, the fine-grained control block
// and everything of rpe_dist.hip are not plain device memory and stay where they are).  rpeh::DevBuf<T> owns a pointer and its
// capacity in bytes and frees in its destructor: a member of rpe_context / rpe_graph goes with its owner, a local with its scope.
// This header includes no HIP header: hipMalloc, hipFree, hipMemcpyAsync, hipStreamSynchronize, hipGetErrorString, their types and
// RPE_OK / RPE_ERR_HIP are the includer's (the HIP runtime in the library, a fake in tests/cpp/devbuf_host.cpp).
#pragma once
#include <cstddef>
#include <utility>

namespace rpeh __attribute__((visibility("hidden"))) {

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// the untyped owner; DevBuf<T> below only adds the pointer's type
class DevMem {
 public:
  DevMem() = default;
  DevMem(DevMem&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  DevMem& operator=(DevMem&& o) noexcept { DevMem old(std::move(*this)); p_ = std::exchange(o.p_, nullptr); cap_ = std::exchange(o.cap_, 0); return *this; }
  ~DevMem() { if (p_) (void)hipFree(p_); }
  size_t bytes() const { return cap_; }

  // at least `bytes` bytes, content not kept.  Enough room: no runtime call.  Otherwise the stream is waited for (a kernel in flight
  // may still use the old array), the old array goes and exactly `bytes` are allocated: growth policies are the callers'.  After a
  // failure the buffer is empty and the next call tries again
  template <class Ctx> int reserve(Ctx* c, size_t bytes) {
    if (p_ && cap_ >= bytes) return RPE_OK;
    if (p_) {
      const hipError_t e = hipStreamSynchronize(c->stream);
      if (e != hipSuccess) return fail(RPE_ERR_HIP, "hipStreamSynchronize: %s", hipGetErrorString(e));
      *this = DevMem();
    }
    return alloc(bytes);
  }
  // allocated on first use, never resized
  template <class Ctx> int once(Ctx*, size_t bytes) { return p_ ? RPE_OK : alloc(bytes); }

  // Larger arrays with the first `keep` bytes of each kept, all or nothing: every new array first, the copies behind one another on
  // the stream, ONE wait, then the old arrays go.  A failure on the way frees what was new and leaves every buffer as it was
  struct Grow { DevMem* buf; size_t keep, bytes; };
  template <class Ctx, size_t N> static int regrow(Ctx* c, const char* what, const Grow (&g)[N]) {
    DevMem q[N];
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < N && e == hipSuccess; i++) {
      if ((e = hipMalloc(&q[i].p_, g[i].bytes)) == hipSuccess) q[i].cap_ = g[i].bytes; else q[i].p_ = nullptr;
    }
    for (size_t i = 0; i < N && e == hipSuccess; i++)
      if (g[i].buf->p_ && g[i].keep) e = hipMemcpyAsync(q[i].p_, g[i].buf->p_, g[i].keep, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(RPE_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    for (size_t i = 0; i < N; i++) *g[i].buf = std::move(q[i]);
    return RPE_OK;
  }

 protected:
  void* p_ = nullptr;
  size_t cap_ = 0;

 private:
  // (a request for 0 bytes still yields a pointer: a null one means "not there" everywhere in the host units)
  int alloc(size_t bytes) {
    const hipError_t e = hipMalloc(&p_, bytes ? bytes : 8);
    if (e != hipSuccess) { p_ = nullptr; return fail(RPE_ERR_HIP, "hipMalloc of %zu bytes: %s", bytes, hipGetErrorString(e)); }
    cap_ = bytes;
    return RPE_OK;
  }
};

template <class T> class DevBuf : public DevMem {
 public:
  T* get() const { return static_cast<T*>(p_); }
  operator T*() const { return get(); }   // reads like the raw pointer it replaces: kernel arguments, offsets, null tests
  T* operator->() const { return get(); }
};

}  // namespace rpeh
