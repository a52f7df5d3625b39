// agz_common.h -- shared host-side helpers of libagz (error plumbing, HIP checks).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <utility>

#include "../../include/agz.h"
#include "../../include/agz_debug.h"

namespace agz {

struct Error : std::runtime_error {
  agz_status status;
  Error(agz_status s, const std::string& m) : std::runtime_error(m), status(s) {}
};

inline std::string fmt(const char* f, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof(buf), f, ap);
  va_end(ap);
  return buf;
}

#define AGZ_HIP(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      throw ::agz::Error(AGZ_HIP_ERROR, ::agz::fmt("%s failed: %s (%s:%d)", #expr,            \
                                                   hipGetErrorString(_e), __FILE__, __LINE__)); \
  } while (0)

#define AGZ_REQUIRE(cond, status, ...)                                  \
  do {                                                                  \
    if (!(cond)) throw ::agz::Error((status), ::agz::fmt(__VA_ARGS__)); \
  } while (0)

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  void alloc(size_t count) {
    release();
    if (count == 0) return;
    AGZ_HIP(hipMalloc((void**)&p, count * sizeof(T)));
    n = count;
  }
  void ensure(size_t count) {
    if (count > n) alloc(count);
  }
  void swap(DevBuf& o) { std::swap(p, o.p), std::swap(n, o.n); }
  void zero(hipStream_t s) {
    if (p) AGZ_HIP(hipMemsetAsync(p, 0, n * sizeof(T), s));
  }
};

// `b` becomes a buffer of `cap` elements that keeps [from, from + keep) of the old one at its front: copied on `s`,
// waited for, then swapped in (the old buffer is freed)
template <class T>
void regrow(DevBuf<T>& b, size_t cap, size_t from, size_t keep, hipStream_t s) {
  DevBuf<T> nb;
  nb.alloc(cap);
  if (keep) AGZ_HIP(hipMemcpyAsync(nb.p, b.p + from, sizeof(T) * keep, hipMemcpyDeviceToDevice, s));
  AGZ_HIP(hipStreamSynchronize(s));
  nb.swap(b);
}

// ---- host <-> device staging, written once.  Every copy is asynchronous on the caller's stream and counts ELEMENTS of
// T: the byte count comes from the type, and host and device pointers must agree on it.  The rules the callers keep:
//  * a copy from or into host memory that the caller owns on its stack or in a vector is followed by a
//    hipStreamSynchronize before that memory dies (fetch / put do it themselves);
//  * several downloads of one entry point share one synchronise: download() never waits;
//  * stage() grows the buffer first, so within one call every pointer into a staging buffer is taken after the last
//    ensure()/stage() of that buffer; a buffer that plays several roles in one call is ensure()d once for all of them
//    and filled with upload() at offsets;
//  * n == 0 copies nothing, and download() into a NULL host pointer is a no-op (an output the caller does not want).
template <class T>
void upload(T* dev, const T* host, size_t n, hipStream_t s) {
  if (n) AGZ_HIP(hipMemcpyAsync(dev, host, sizeof(T) * n, hipMemcpyHostToDevice, s));
}
template <class T>
void download(T* host, const T* dev, size_t n, hipStream_t s) {
  if (host && n) AGZ_HIP(hipMemcpyAsync(host, dev, sizeof(T) * n, hipMemcpyDeviceToHost, s));
}
// n elements into a staging buffer, grown as needed; the device pointer to use from here on
template <class T>
T* stage(DevBuf<T>& buf, const T* host, size_t n, hipStream_t s) {
  buf.ensure(n);
  upload(buf.p, host, n, s);
  return buf.p;
}
// one object down (or up) and the synchronise: the accessors that read or write exactly one thing
template <class T>
T fetch(const T* dev, hipStream_t s) {
  T v;
  download(&v, dev, 1, s);
  AGZ_HIP(hipStreamSynchronize(s));
  return v;
}
template <class T>
void put(T* dev, const T& v, hipStream_t s) {
  upload(dev, &v, 1, s);
  AGZ_HIP(hipStreamSynchronize(s));
}

inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

}  // namespace agz
