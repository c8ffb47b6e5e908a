/*
 * host_hip.h — move-only owners of the host runtime's HIP resources (device
 * buffer, pinned host buffer, stream, event: each frees in its destructor),
 * the one grow-a-buffer routine, and the environment-knob readers.
 *
 * The owners free on whatever device is current: the holder selects the
 * device before it lets them go (pht_ctx_destroy, group_destroy).
 */
#ifndef PHT_HOST_HIP_H
#define PHT_HOST_HIP_H

#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#pragma GCC visibility push(hidden)
namespace pht {
namespace host {

/* environment knobs: read where the value is used, never cached (tests and
 * tools change some of them between sweeps of one process) */
inline int env_int(const char *name, int dflt) {
  const char *e = getenv(name);
  return e ? atoi(e) : dflt;
}
inline long env_long(const char *name, long dflt) {
  const char *e = getenv(name);
  return e ? atol(e) : dflt;
}
inline bool env_is(const char *name, const char *value) {
  const char *e = getenv(name);
  return e && !strcmp(e, value);
}

/* one HIP handle (a pointer type H), released by Free */
template <class H, hipError_t (*Free)(H)>
class Owned {
 protected:
  H h_ = nullptr;

 public:
  Owned() = default;
  Owned(Owned &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  Owned &operator=(Owned &&o) noexcept {
    if (this != &o) {
      reset();
      h_ = o.h_;
      o.h_ = nullptr;
    }
    return *this;
  }
  ~Owned() { reset(); }
  void reset() {
    if (h_) (void)Free(h_);
    h_ = nullptr;
  }
  H get() const { return h_; }
  explicit operator bool() const { return h_ != nullptr; }
};

struct Stream : Owned<hipStream_t, hipStreamDestroy> {
  hipError_t create() { return hipStreamCreateWithFlags(&h_, hipStreamNonBlocking); }
};
struct Event : Owned<hipEvent_t, hipEventDestroy> {
  hipError_t create() { return hipEventCreate(&h_); } /* with timing */
  hipError_t create_untimed() { return hipEventCreateWithFlags(&h_, hipEventDisableTiming); }
};

/* device memory: count elements of T, uninitialised; cap(): that count (0 when empty) */
template <class T>
class DevBuf : public Owned<void *, hipFree> {
  size_t cap_ = 0;

 public:
  hipError_t alloc(size_t count) {
    reset();
    const hipError_t e = hipMalloc(&h_, sizeof(T) * count);
    if (e != hipSuccess) h_ = nullptr;
    cap_ = count;
    return e;
  }
  T *get() const { return static_cast<T *>(h_); }
  size_t cap() const { return h_ ? cap_ : 0; }
};

/* pinned host memory (hipHostMalloc flags); mapped: with its device alias */
template <class T>
class PinnedBuf : public Owned<void *, hipHostFree> {
  void *dev_ = nullptr;

 public:
  hipError_t alloc(size_t count, unsigned flags = 0, bool mapped = false) {
    reset();
    dev_ = nullptr;
    hipError_t e = hipHostMalloc(&h_, sizeof(T) * count, flags);
    if (e != hipSuccess) h_ = nullptr;
    if (e == hipSuccess && mapped && (e = hipHostGetDevicePointer(&dev_, h_, 0)) != hipSuccess) reset();
    return e;
  }
  T *get() const { return static_cast<T *>(h_); }
  T *dev() const { return h_ ? static_cast<T *>(dev_) : nullptr; } /* the mapped alias, if mapped */
};

/* the grow pattern: when need exceeds buf.cap(), free it and allocate
 * max(need, headroom) (contents are not kept).  On failure the buffer is
 * empty and its cap() is 0. */
template <class T>
hipError_t ensure(DevBuf<T> &buf, size_t need, size_t headroom = 0) {
  return need <= buf.cap() ? hipSuccess : buf.alloc(std::max(need, headroom));
}

}  // namespace host
}  // namespace pht
#pragma GCC visibility pop

#endif
