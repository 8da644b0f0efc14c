// hip_raii.h — move-only owners of the host layer's HIP resources (capi.cpp, multi.cpp): device
// buffers, events, streams, host-mapped words and pools of timing events. None of them knows a
// device: the containing object's destructor makes the right device current (and drains what may
// still run) before its members go.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <mutex>
#include <utility>
#include <vector>

namespace yart_impl {

inline hipError_t drain(const hipStream_t* streams, size_t n) {
  hipError_t e = hipSuccess;
  for (size_t i = 0; i < n && e == hipSuccess; ++i) e = hipStreamSynchronize(streams[i]);
  return e;
}

// A hipMalloc block and its byte count.
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { (void)release(); p_ = std::exchange(o.p_, nullptr); n_ = std::exchange(o.n_, 0); }
    return *this;
  }
  ~DevBuf() { (void)release(); }
  hipError_t alloc(size_t bytes) {  // gives up what it held, whether or not the new block comes
    hipError_t e = release();
    if (e == hipSuccess && (e = hipMalloc(&p_, bytes)) == hipSuccess) n_ = bytes;
    else p_ = nullptr;
    return e;
  }
  hipError_t release() {
    const hipError_t e = p_ ? hipFree(p_) : hipSuccess;
    p_ = nullptr; n_ = 0;
    return e;
  }
  // Grow on demand: nothing if the block holds `bytes`; otherwise drain the streams whose queued work
  // may still use the old block (none, if there is no old block), release it, allocate the new one.
  hipError_t reserve(size_t bytes, const hipStream_t* streams, size_t n) {
    if (n_ >= bytes) return hipSuccess;
    if (p_)
      if (hipError_t e = drain(streams, n)) return e;
    return alloc(bytes);
  }
  hipError_t reserve(size_t bytes, std::initializer_list<hipStream_t> streams) {
    return reserve(bytes, streams.begin(), streams.size());
  }
  template <class T> T* get() const { return static_cast<T*>(p_); }
  size_t bytes() const { return n_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  void* p_ = nullptr;
  size_t n_ = 0;
};

// An event or a stream: a handle and the call that destroys it.
template <class H, hipError_t (*Destroy)(H)>
class Handle {
 public:
  Handle() = default;
  Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  Handle& operator=(Handle&& o) noexcept {
    if (this != &o) { reset(); h_ = std::exchange(o.h_, nullptr); }
    return *this;
  }
  ~Handle() { reset(); }
  void reset() { if (h_) (void)Destroy(h_); h_ = nullptr; }
  operator H() const { return h_; }

 protected:
  H h_ = nullptr;
};
struct Event : Handle<hipEvent_t, hipEventDestroy> {
  hipError_t create(unsigned flags = hipEventDisableTiming) { reset(); return hipEventCreateWithFlags(&h_, flags); }
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> {  // library-owned streams are all non-blocking
  hipError_t create() { reset(); return hipStreamCreateWithFlags(&h_, hipStreamNonBlocking); }
};

// Host memory the device writes and the host polls (mapped + coherent), with the device's pointer.
class HostMapped {
 public:
  HostMapped() = default;
  HostMapped(HostMapped&& o) noexcept : h_(std::exchange(o.h_, nullptr)), d_(std::exchange(o.d_, nullptr)) {}
  HostMapped& operator=(HostMapped&& o) noexcept {
    if (this != &o) { release(); h_ = std::exchange(o.h_, nullptr); d_ = std::exchange(o.d_, nullptr); }
    return *this;
  }
  ~HostMapped() { release(); }
  hipError_t alloc(size_t bytes) {
    release();
    hipError_t e = hipHostMalloc(&h_, bytes, hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) { h_ = nullptr; return e; }
    if ((e = hipHostGetDevicePointer(&d_, h_, 0)) != hipSuccess) release();
    return e;
  }
  void release() { if (h_) (void)hipHostFree(h_); h_ = d_ = nullptr; }
  uint32_t* host() const { return static_cast<uint32_t*>(h_); }
  uint32_t* device() const { return static_cast<uint32_t*>(d_); }

 private:
  void *h_ = nullptr, *d_ = nullptr;
};

// Recycled timing events. take() leases n of them (idle ones first, new ones after); a lease gives
// its events back when it goes, so an enqueue that fails half way loses none, and a list of frames
// not yet read is a list of leases: reading it and letting it go recycles the events. The pool
// outlives its leases (declare it before whatever holds them).
class EventPool {
 public:
  class Lease {
   public:
    Lease() = default;
    Lease(Lease&& o) noexcept : pool_(o.pool_), ev_(std::exchange(o.ev_, {})) {}
    Lease& operator=(Lease&& o) noexcept {  // what this one held goes back with `o`
      std::swap(pool_, o.pool_);
      ev_.swap(o.ev_);
      return *this;
    }
    ~Lease() {
      if (ev_.empty()) return;
      std::lock_guard<std::mutex> lk(pool_->mu_);
      pool_->idle_.insert(pool_->idle_.end(), ev_.begin(), ev_.end());
    }
    hipEvent_t operator[](size_t i) const { return ev_[i]; }
    size_t size() const { return ev_.size(); }

   private:
    friend class EventPool;
    EventPool* pool_ = nullptr;
    std::vector<hipEvent_t> ev_;
  };

  EventPool() = default;
  EventPool(const EventPool&) = delete;
  EventPool& operator=(const EventPool&) = delete;
  ~EventPool() { clear(); }
  hipError_t take(size_t n, Lease& out) {  // on the current device
    Lease l;
    l.pool_ = this;
    l.ev_.reserve(n);
    {
      std::lock_guard<std::mutex> lk(mu_);
      for (; l.ev_.size() < n && !idle_.empty(); idle_.pop_back()) l.ev_.push_back(idle_.back());
    }
    while (l.ev_.size() < n) {
      hipEvent_t e;
      if (hipError_t err = hipEventCreate(&e)) return err;  // `l` gives back what it has
      l.ev_.push_back(e);
    }
    out = std::move(l);
    return hipSuccess;
  }
  void clear() {  // destroys the idle events
    std::lock_guard<std::mutex> lk(mu_);
    for (hipEvent_t e : idle_) (void)hipEventDestroy(e);
    idle_.clear();
  }

 private:
  std::mutex mu_;
  std::vector<hipEvent_t> idle_;
};

}  // namespace yart_impl
