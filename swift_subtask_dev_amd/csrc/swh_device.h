// swh_device.h — the owners of libswifthip's HIP resources, and the one
// readback of a small device record that every queued result goes through.
//
// The ownership rule: a device buffer, a pinned buffer, an event, a stream or
// a hipFFT plan is held by exactly one object of a type below, which frees it
// in its destructor. The owners are move-only; a struct that holds them needs
// no teardown code of its own, and `delete` of a space is its whole release.
// Members are destroyed in reverse order of declaration, so a struct declares
// its owned stream first: it goes after everything recorded on it.
//
// No object with static or thread-local storage duration may hold an owner:
// its destructor would run after the HIP runtime is gone. There is none.
//
// Host code only (hip_runtime_api.h, no kernels): a plain host compiler
// builds this header with -D__HIP_PLATFORM_AMD__, which is how its test runs
// it against malloc-backed fakes of the HIP calls.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstring>
#include <utility>

#include "swifthip.h"

namespace swh {

// ---------------------------------------------------------------------------
// Errors: thread-local message + status codes, no aborts.
// ---------------------------------------------------------------------------
void set_error(const char* fmt, ...);

#define SWH_HIP(call)                                                           \
  do {                                                                          \
    hipError_t _e = (call);                                                     \
    if (_e != hipSuccess) {                                                     \
      ::swh::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e),   \
                       __FILE__, __LINE__);                                     \
      return (_e == hipErrorOutOfMemory) ? SWH_ERR_OOM : SWH_ERR_HIP;           \
    }                                                                           \
  } while (0)

#define SWH_TRY(expr)                      \
  do {                                     \
    swh_status _s = (expr);                \
    if (_s != SWH_OK) return _s;           \
  } while (0)

// A move-only handle that Destroy() takes back: events, streams, hipFFT plans.
template <typename H, auto Destroy>
struct Handle {
  H h = H{};
  Handle() = default;
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
  Handle(Handle&& o) noexcept : h(o.h) { o.h = H{}; }
  Handle& operator=(Handle&& o) noexcept {
    if (this != &o) {
      reset();
      h = o.h;
      o.h = H{};
    }
    return *this;
  }
  ~Handle() { reset(); }
  void reset() {
    if (h) (void)Destroy(h);
    h = H{};
  }
  // the empty handle's address, for the create call to fill
  H* put() {
    reset();
    return &h;
  }
  operator H() const { return h; }
};

using Stream = Handle<hipStream_t, hipStreamDestroy>;

struct Event : Handle<hipEvent_t, hipEventDestroy> {
  // created on first use (flags: hipEventDefault, hipEventDisableTiming)
  swh_status ensure(unsigned flags = hipEventDefault) {
    if (!h) SWH_HIP(hipEventCreateWithFlags(&h, flags));
    return SWH_OK;
  }
};

// Growable device buffer (never shrinks; reused across calls so the loops do
// no allocation once warm).
struct DevBuf {
  void* ptr = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr, o.bytes = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      ptr = o.ptr, bytes = o.bytes;
      o.ptr = nullptr, o.bytes = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  swh_status reserve(size_t b) {
    if (b <= bytes) return SWH_OK;
    reset();
    size_t nb = b < 256 ? 256 : b;
    hipError_t e = hipMalloc(&ptr, nb);
    if (e != hipSuccess) {
      ptr = nullptr;
      set_error("hipMalloc(%zu) failed: %s", nb, hipGetErrorString(e));
      return SWH_ERR_OOM;
    }
    bytes = nb;
    return SWH_OK;
  }
  // Grow (at least doubling) keeping the first `used` bytes; the stream is
  // waited for before the old buffer goes, whatever work still reads it.
  swh_status grow_keep(size_t need, size_t used, hipStream_t stream) {
    if (need <= bytes) return SWH_OK;
    DevBuf nb;
    SWH_TRY(nb.reserve(need > 2 * bytes ? need : 2 * bytes));
    if (used > 0) SWH_HIP(hipMemcpyAsync(nb.ptr, ptr, used, hipMemcpyDeviceToDevice, stream));
    SWH_HIP(hipStreamSynchronize(stream));
    *this = std::move(nb);
    return SWH_OK;
  }
  template <typename T>
  T* as() const { return reinterpret_cast<T*>(ptr); }

 private:
  void reset() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr, bytes = 0;
  }
};

// Pinned host staging buffer.
struct HostBuf {
  void* ptr = nullptr;
  size_t bytes = 0;
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  HostBuf(HostBuf&& o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr, o.bytes = 0; }
  HostBuf& operator=(HostBuf&& o) noexcept {
    if (this != &o) {
      reset();
      ptr = o.ptr, bytes = o.bytes;
      o.ptr = nullptr, o.bytes = 0;
    }
    return *this;
  }
  ~HostBuf() { reset(); }
  swh_status reserve(size_t b) {
    if (b <= bytes) return SWH_OK;
    reset();
    size_t nb = b < 4096 ? 4096 : b;
    hipError_t e = hipHostMalloc(&ptr, nb, hipHostMallocDefault);
    if (e != hipSuccess) {
      ptr = nullptr;
      set_error("hipHostMalloc(%zu) failed: %s", nb, hipGetErrorString(e));
      return SWH_ERR_OOM;
    }
    bytes = nb;
    return SWH_OK;
  }
  template <typename T>
  T* as() const { return reinterpret_cast<T*>(ptr); }

 private:
  void reset() {
    if (ptr) (void)hipHostFree(ptr);
    ptr = nullptr, bytes = 0;
  }
};

// A small device record, its pinned copy and the event behind the last copy:
// how every queued result reaches the host.
//   pending: a copy (or the work mark() stands behind) is queued and nobody
//            has waited for it; the pinned copy is not the host's yet
//   has:     the pinned copy holds (or will hold, once waited for) a result
// queue() never waits: copies queued back to back on one stream arrive in
// order, so the pinned copy needs no guard between them. The waits are the
// callers': wait() in every _result entry, and on entry of a call that writes
// the pinned copy from the host or grows the record (prepare() with more
// bytes than before frees buffers a pending copy would still use).
struct Readback {
  DevBuf rec;
  HostBuf pinned;
  Event event;
  size_t size = 0;  // bytes of the record: what queue() copies
  bool pending = false, has = false;

  // (the device record last: one that exists has been through a whole prepare)
  swh_status prepare(size_t bytes) {
    SWH_TRY(pinned.reserve(bytes));
    SWH_TRY(event.ensure(hipEventDisableTiming));
    SWH_TRY(rec.reserve(bytes));
    size = bytes;
    return SWH_OK;
  }
  template <typename T>
  T* dev() const { return rec.as<T>(); }
  template <typename T>
  const T* host() const { return pinned.as<const T>(); }
  // the event alone: the record was copied already, `st` still has work of
  // the call whose result it is
  swh_status mark(hipStream_t st) {
    SWH_HIP(hipEventRecord(event, st));
    pending = has = true;
    return SWH_OK;
  }
  swh_status queue(hipStream_t st) {
    SWH_HIP(hipMemcpyAsync(pinned.ptr, rec.ptr, size, hipMemcpyDeviceToHost, st));
    return mark(st);
  }
  swh_status wait() {
    if (!pending) return SWH_OK;
    SWH_HIP(hipEventSynchronize(event));
    pending = false;
    return SWH_OK;
  }
  // the result of an empty set, written by the host (src == nullptr: zeros);
  // a pending copy lands first
  swh_status set_host(const void* src, size_t bytes) {
    SWH_TRY(wait());
    SWH_TRY(pinned.reserve(bytes));
    if (src)
      std::memcpy(pinned.ptr, src, bytes);
    else
      std::memset(pinned.ptr, 0, bytes);
    has = true;
    return SWH_OK;
  }
  void invalidate() { pending = has = false; }
};

// HIP events around the last launch of each of N stages.
template <int N>
struct StageTimer {
  Event ev[N][2];
  bool timed[N] = {};
  swh_status begin(int k, hipStream_t st) {
    for (Event& e : ev[k]) SWH_TRY(e.ensure());
    SWH_HIP(hipEventRecord(ev[k][0], st));
    return SWH_OK;
  }
  swh_status end(int k, hipStream_t st) {
    SWH_HIP(hipEventRecord(ev[k][1], st));
    timed[k] = true;
    return SWH_OK;
  }
  // ms[k]: the last launch of stage k, -1 if it never ran; waits for it
  swh_status read(float* ms) {
    for (int k = 0; k < N; k++) {
      ms[k] = -1.f;
      if (!timed[k]) continue;
      SWH_HIP(hipEventSynchronize(ev[k][1]));
      SWH_HIP(hipEventElapsedTime(&ms[k], ev[k][0], ev[k][1]));
    }
    return SWH_OK;
  }
};

}  // namespace swh
