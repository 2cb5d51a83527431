// Host-side owners of HIP resources for the encode pipelines (host code
// only; no kernels). A pipeline declares them in this order —
// UseDevice, Arena, FrameUploader, Streams, Events, CompactReadback —
// so that destruction drains every stream before any memory goes away.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#define HIP_CHECK(expr)                                                    \
  do {                                                                     \
    hipError_t _e = (expr);                                                \
    if (_e != hipSuccess) {                                                \
      throw std::runtime_error(std::string("HIP error: ") +                \
                               hipGetErrorString(_e) + " at " #expr);      \
    }                                                                      \
  } while (0)

namespace hipflux {

// Encode worker pool size, capped at 16: the per-frame batches are small,
// and waking a hardware_concurrency/2-sized pool (128 threads on a
// 256-core box) costs more in cv wakeups than the work itself.
inline unsigned encode_pool_threads() {
  return std::min(16u, std::max(2u, std::thread::hardware_concurrency() / 2));
}

inline double now_us() {
  return std::chrono::duration<double, std::micro>(
             std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

// First member of a pipeline: selects the device before the members
// after it create their streams and events on it.
struct UseDevice {
  explicit UseDevice(int gpu_id) {
    HIP_CHECK(hipSetDevice(std::max(0, gpu_id)));
  }
};

// Non-blocking stream; drained, then destroyed, with its owner.
class Stream {
 public:
  Stream() { HIP_CHECK(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking)); }
  Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() {
    if (!s_) return;
    (void)hipStreamSynchronize(s_);
    (void)hipStreamDestroy(s_);
  }
  operator hipStream_t() const { return s_; }
  void sync() const { HIP_CHECK(hipStreamSynchronize(s_)); }

 private:
  hipStream_t s_ = nullptr;
};

class Event {
 public:
  explicit Event(unsigned flags = hipEventDisableTiming) {
    HIP_CHECK(hipEventCreateWithFlags(&e_, flags));
  }
  Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() {
    if (e_) (void)hipEventDestroy(e_);
  }
  operator hipEvent_t() const { return e_; }
  void sync() const { HIP_CHECK(hipEventSynchronize(e_)); }

 private:
  hipEvent_t e_ = nullptr;
};

// Owns every device and pinned-host buffer of one allocation epoch (for
// the pipelines: one resolution). The pipeline keeps plain pointers,
// because the launchers take plain pointers; the arena remembers where
// they live and nulls them in release(), so a later allocation that
// throws leaves null pointers behind, never dangling ones. The owner of
// those pointers must therefore not move while the arena holds buffers.
class Arena {
 public:
  Arena() = default;
  Arena(const Arena&) = delete;
  Arena& operator=(const Arena&) = delete;
  ~Arena() { release(); }

  template <typename T>
  void dev(T*& slot, size_t n) {
    void* p = nullptr;
    HIP_CHECK(hipMalloc(&p, n * sizeof(T)));
    track(slot, p, false);
  }
  template <typename T>
  void pinned(T*& slot, size_t n) {
    void* p = nullptr;
    HIP_CHECK(hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault));
    track(slot, p, true);
  }
  // The caller has drained every stream that may still touch a buffer.
  void release() {
    for (const Buf& b : bufs_) {
      b.clear(b.slot);
      (void)(b.host ? hipHostFree(b.p) : hipFree(b.p));
    }
    bufs_.clear();
  }

 private:
  struct Buf {
    void* p;
    void* slot;              // the owner's T* member that holds p
    void (*clear)(void*);    // nulls *slot with its real type
    bool host;
  };
  template <typename T>
  void track(T*& slot, void* p, bool host) {
    slot = static_cast<T*>(p);
    bufs_.push_back(
        {p, &slot, [](void* s) { *static_cast<T**>(s) = nullptr; }, host});
  }
  std::vector<Buf> bufs_;
};

// Makes a caller-owned frame DMA-able. The capture buffer is registered
// once (zero-copy DMA afterwards); if registration fails the frame is
// staged through a pinned buffer instead — an unpinned async copy
// silently degrades to a slow sync path. Registrations remember their
// length: a longer frame at a known address (resolution change, reused
// allocation) is registered afresh, never sent with only its head pinned.
class FrameUploader {
 public:
  FrameUploader() = default;
  FrameUploader(const FrameUploader&) = delete;
  FrameUploader& operator=(const FrameUploader&) = delete;
  ~FrameUploader() {
    for (auto& kv : reg_)
      if (kv.second.ok) (void)hipHostUnregister(kv.first);
    if (stage_) (void)hipHostFree(stage_);
  }

  // The pointer to copy `bytes` from: `src` itself, or the staging copy.
  // No copy from `src` or the staging buffer may still be in flight (the
  // pipelines wait for a frame's H2D before they take the next frame).
  const uint8_t* source(const uint8_t* src, size_t bytes) {
    void* base = const_cast<uint8_t*>(src);
    auto it = reg_.find(base);
    if (it == reg_.end() || it->second.bytes < bytes) {
      if (it != reg_.end() && it->second.ok) (void)hipHostUnregister(base);
      const bool ok =
          hipHostRegister(base, bytes, hipHostRegisterDefault) == hipSuccess;
      if (!ok) (void)hipGetLastError();  // clear; stage instead
      it = reg_.insert_or_assign(base, Reg{bytes, ok}).first;
    }
    if (it->second.ok) return src;
    if (stage_bytes_ < bytes) {
      if (stage_) (void)hipHostFree(stage_);
      stage_ = nullptr;
      stage_bytes_ = 0;
      HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&stage_), bytes,
                              hipHostMallocDefault));
      stage_bytes_ = bytes;
    }
    std::memcpy(stage_, src, bytes);
    return stage_;
  }

 private:
  struct Reg {
    size_t bytes;
    bool ok;
  };
  std::map<void*, Reg> reg_;
  uint8_t* stage_ = nullptr;
  size_t stage_bytes_ = 0;
};

// Adaptive compacted read-back of `rows` fixed-stride rows of T whose
// used prefix is only known on the device: read() copies a capped prefix
// of every row (the whole rows while the cap covers the stride) and
// returns the cap it used; settle(), once the per-row use is on the host,
// fetches exactly the rows that outgrew that cap — on a stream of its
// own, so they never queue behind the next frame's work — and sets the
// cap for the next frame.
template <typename T>
class CompactReadback {
 public:
  // stride and first cap, in elements of T; call on every (re)allocation
  void reset(int stride, int cap) {
    stride_ = stride;
    cap_ = cap;
  }
  int read(T* h, const T* d, int rows, hipStream_t stream) const {
    const int cap = std::min(stride_, cap_);
    const size_t pitch = static_cast<size_t>(stride_) * sizeof(T);
    if (cap >= stride_) {
      HIP_CHECK(hipMemcpyAsync(h, d, rows * pitch, hipMemcpyDeviceToHost,
                               stream));
    } else {
      HIP_CHECK(hipMemcpy2DAsync(h, pitch, d, pitch, cap * sizeof(T), rows,
                                 hipMemcpyDeviceToHost, stream));
    }
    return cap;
  }
  // used(row) -> elements of that row to keep; next_cap(max used) -> cap.
  // The device rows must still hold this frame's data.
  template <typename Used, typename NextCap>
  void settle(T* h, const T* d, int rows, int cap, Used used,
              NextCap next_cap) {
    int max_used = 0;
    bool fix = false;
    for (int r = 0; r < rows; ++r) {
      const int n = used(r);
      max_used = std::max(max_used, n);
      if (n <= cap) continue;
      const size_t off = static_cast<size_t>(r) * stride_;
      HIP_CHECK(hipMemcpyAsync(h + off, d + off, n * sizeof(T),
                               hipMemcpyDeviceToHost, fix_));
      fix = true;
    }
    if (fix) fix_.sync();
    cap_ = next_cap(max_used);
  }

 private:
  Stream fix_;
  int stride_ = 0;
  int cap_ = 0;
};

}  // namespace hipflux
