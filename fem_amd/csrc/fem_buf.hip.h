// fem_buf.hip.h — who owns what in libfemhip.so: device and pinned host memory (Buf), events (Event, EventPool) and streams
// (Stream).  Each frees what it holds when it goes; nothing else in csrc/ calls hipMalloc, hipFree and their kin.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace femb {

enum class Mem { Device, Pinned };
// How a buffer that is too small picks its new size: part of its type, so that every buffer keeps the rule it was written
// with (the sizes asked of the runtime are what the regrow tests, FEM_TEST_TINY_BUFFERS, and a job's memory budget rest on).
enum class Grow {
  Exact,    // the elements asked for
  Half,     // ... or half as many again as it held, whichever is more, and one at least (a slot's staging buffers)
  Quarter,  // a quarter more bytes than asked for, 256 at least (the tail's and the compressor's buffers)
};

inline std::atomic<uint64_t> g_live_bytes[2];  // [Mem]: bytes held by all Bufs of the process (fem_dbg_live_bytes)

template <typename T, Mem M = Mem::Device, Grow G = Grow::Exact>
class Buf {
 public:
  Buf() = default;
  Buf(const Buf &) = delete;
  Buf &operator=(const Buf &) = delete;
  Buf(Buf &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr, o.bytes_ = 0; }
  Buf &operator=(Buf &&o) noexcept {
    if (this != &o) {
      release();
      p_ = o.p_, bytes_ = o.bytes_;
      o.p_ = nullptr, o.bytes_ = 0;
    }
    return *this;
  }
  ~Buf() { release(); }

  operator T *() const { return p_; }
  T *get() const { return p_; }
  size_t bytes() const { return bytes_; }
  size_t size() const { return bytes_ / sizeof(T); }  // elements

  void release() {
    if (p_) {
      (void)(M == Mem::Pinned ? hipHostFree(p_) : hipFree(p_));
      g_live_bytes[(int)M].fetch_sub(bytes_, std::memory_order_relaxed);
    }
    p_ = nullptr, bytes_ = 0;
  }
  // Room for n elements.  What it held is lost when it has to move; on failure it is empty — but for a device buffer under
  // Grow::Half, which asks for its new memory first and stays as it was when there is none (the batch staged in it before
  // can still be mapped).
  hipError_t ensure(size_t n) {
    if (p_ && n <= size()) return hipSuccess;
    const size_t want = new_bytes(n);
    if (M == Mem::Device && G == Grow::Half) {
      Buf fresh;
      const hipError_t e = fresh.take(want);
      if (e == hipSuccess) *this = std::move(fresh);
      return e;
    }
    release();
    return take(want);
  }
  // ensure(n) that keeps the first `used` elements (waits for `stream` when it has to move them; device memory)
  hipError_t ensure_keep(size_t n, size_t used, hipStream_t stream) {
    if (p_ && n <= size()) return hipSuccess;
    Buf fresh;
    hipError_t e = fresh.take(new_bytes(n));
    if (e != hipSuccess) return e;
    if (p_ && used) e = hipMemcpyAsync(fresh.p_, p_, used * sizeof(T), hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess) *this = std::move(fresh);
    return e;
  }

 private:
  size_t new_bytes(size_t n) const {
    if (G == Grow::Quarter) return std::max<size_t>(n * sizeof(T) + n * sizeof(T) / 4, 256);
    return G == Grow::Half ? std::max<size_t>({n, size() + size() / 2, (size_t)1}) * sizeof(T) : n * sizeof(T);
  }
  hipError_t take(size_t want) {  // (empty before)
    void *q = nullptr;
    const hipError_t e = M == Mem::Pinned ? hipHostMalloc(&q, want, hipHostMallocDefault) : hipMalloc(&q, want);
    if (e != hipSuccess) return e;
    p_ = (T *)q, bytes_ = q ? want : 0;
    g_live_bytes[(int)M].fetch_add(bytes_, std::memory_order_relaxed);
    return hipSuccess;
  }
  T *p_ = nullptr;
  size_t bytes_ = 0;
};
template <typename T>
using PinBuf = Buf<T, Mem::Pinned>;

// Arrays that share one capacity (a slot's four candidate arrays, a result's pinned triple): n elements each, new — or, where
// one of them cannot be had, none of them holds anything, and the caller does not publish the capacity.
template <typename... B>
hipError_t alloc_all(size_t n, B &...b) {
  (b.release(), ...);
  hipError_t e = hipSuccess;
  (void)(((e = b.ensure(n)) == hipSuccess) && ...);
  if (e != hipSuccess) (b.release(), ...);
  return e;
}

struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event &) = delete;
  Event &operator=(const Event &) = delete;
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  operator hipEvent_t() const { return e; }
  hipError_t create(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }  // (once)
};

struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream &) = delete;
  Stream &operator=(const Stream &) = delete;
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
  operator hipStream_t() const { return s; }
  hipError_t create(unsigned flags) { return hipStreamCreateWithFlags(&s, flags); }
  hipError_t create(unsigned flags, int priority) { return hipStreamCreateWithPriority(&s, flags, priority); }
};

// Timing events, handed out and taken back (a launch is timed between two of them; they are made as they are first needed)
struct EventPool {
  std::vector<hipEvent_t> idle;
  EventPool() = default;
  EventPool(const EventPool &) = delete;
  EventPool &operator=(const EventPool &) = delete;
  ~EventPool() {
    for (hipEvent_t e : idle) (void)hipEventDestroy(e);
  }
  hipEvent_t get() {
    hipEvent_t e = nullptr;
    if (idle.empty()) {
      (void)hipEventCreate(&e);
    } else {
      e = idle.back();
      idle.pop_back();
    }
    return e;
  }
  void put(hipEvent_t e) { idle.push_back(e); }
  hipError_t fill(size_t n) {  // n idle events at least, made now
    hipError_t err = hipSuccess;
    for (hipEvent_t e = nullptr; idle.size() < n && (err = hipEventCreate(&e)) == hipSuccess;) idle.push_back(e);
    return err;
  }
};

}  // namespace femb
