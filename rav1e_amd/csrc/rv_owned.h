// rv_owned.h -- internal, host only: the one owner of what the HIP runtime
// hands out to a replay instance or a lookahead engine.  Each call creates one
// object, records it and returns it; a failed call latches `failed` and returns
// null (checked once after a run of creations).  One dev() is one hipMalloc.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>

namespace rv {

// What a fresh device buffer holds: whatever hipMalloc returns, zeros, or Byte(v)
enum class Fill : int { None = -1, Zero = 0 };
constexpr Fill Byte(unsigned char v) { return Fill(v); }

struct Owned {
  std::vector<void *> device, host;
  std::vector<hipEvent_t> events;
  std::vector<hipStream_t> streams;
  size_t device_bytes = 0;
  bool failed = false;

  // count elements of T (16 bytes for none); the fill is queued on st
  template <class T>
  T *dev(size_t count, Fill fill, hipStream_t st) {
    const size_t bytes = count * sizeof(T);
    void *p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) return fail<T *>();
    device.push_back(p);
    device_bytes += bytes ? bytes : 16;
    if (fill != Fill::None && hipMemsetAsync(p, (int)fill, bytes, st) != hipSuccess) return fail<T *>();
    return static_cast<T *>(p);
  }
  template <class T>
  T *pinned(size_t count, unsigned flags) {
    void *p = nullptr;
    if (hipHostMalloc(&p, count * sizeof(T), flags) != hipSuccess) return fail<T *>();
    host.push_back(p);
    return static_cast<T *>(p);
  }
  hipEvent_t event(unsigned flags) {
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, flags) != hipSuccess) return fail<hipEvent_t>();
    events.push_back(e);
    return e;
  }
  hipStream_t stream() {  // non-blocking
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return fail<hipStream_t>();
    streams.push_back(s);
    return s;
  }
  // (the caller has drained every stream that may still use any of it)
  void release() {
    for (void *p : device) (void)hipFree(p);
    for (void *p : host) (void)hipHostFree(p);
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    for (hipStream_t s : streams) (void)hipStreamDestroy(s);
    *this = Owned();
  }

 private:
  template <class P>
  P fail() {
    failed = true;
    return nullptr;
  }
};

}  // namespace rv
