// Owners of the HIP resources a context holds (not installed).  Each is move-only, empty when
// default-constructed (no HIP call, no current device needed) and releases what it holds in its
// destructor.  None of them waits for the GPU: whoever frees or regrows a resource first waits for
// its last reader, at the call site, where the stream or event to wait for is known.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace pgh_detail {

// One ordering event (hipEventDisableTiming); reads as the hipEvent_t it holds.
struct Event {
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : ev(std::exchange(o.ev, nullptr)) {}
    Event& operator=(Event&& o) noexcept { std::swap(ev, o.ev); return *this; }
    ~Event() { if (ev) (void)hipEventDestroy(ev); }
    hipError_t make() { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
    operator hipEvent_t() const { return ev; }
};

// One non-blocking stream; reads as the hipStream_t it holds.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream&& o) noexcept : s(std::exchange(o.s, nullptr)) {}
    Stream& operator=(Stream&& o) noexcept { std::swap(s, o.s); return *this; }
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t make() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    operator hipStream_t() const { return s; }
};

// Events of one kind, lent out and taken back.  The pool owns every event it ever made, wherever
// it is at the moment, so nothing has to be handed back before the pool goes.  An event in the free
// list is referenced by nothing; one that an earlier hipStreamWaitEvent captured may be recorded
// again (the wait took the record it saw).
class EventPool {
  public:
    explicit EventPool(unsigned flags) : flags_(flags) {}
    EventPool(EventPool&&) = default;  // (a moved-from vector is empty)
    ~EventPool() { for (hipEvent_t e : all_) (void)hipEventDestroy(e); }
    hipEvent_t take() {  // nullptr: hipEventCreateWithFlags failed
        hipEvent_t e = nullptr;
        if (!free_.empty()) { e = free_.back(); free_.pop_back(); return e; }
        if (hipEventCreateWithFlags(&e, flags_) != hipSuccess) return nullptr;
        all_.push_back(e);
        return e;
    }
    void give(hipEvent_t e) { free_.push_back(e); }
    bool fill(std::vector<hipEvent_t>& v, size_t n) {  // v at least n events long, for good
        for (hipEvent_t e; v.size() < n; v.push_back(e))
            if (!(e = take())) return false;
        return true;
    }

  private:
    unsigned flags_;
    std::vector<hipEvent_t> all_, free_;
};

// A device (hipMalloc) or page-locked host (hipHostMalloc) allocation and its capacity in bytes.
class Buf {
  public:
    Buf(Buf&& o) noexcept : pinned_(o.pinned_), p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    Buf& operator=(Buf&& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); return *this; }
    ~Buf() { reset(); }
    // At least `bytes`: nothing when the capacity suffices, else free + allocate.  false: the
    // allocation failed (HIP's sticky error cleared) and the owner is empty.
    bool reserve(size_t bytes, unsigned host_flags = hipHostMallocDefault) {
        if (bytes <= cap_) return true;
        reset();
        if ((pinned_ ? hipHostMalloc(&p_, bytes, host_flags) : hipMalloc(&p_, bytes)) != hipSuccess) {
            (void)hipGetLastError();
            p_ = nullptr;
            return false;
        }
        cap_ = bytes;
        return true;
    }
    bool reserve_geometric(size_t bytes) { return bytes <= cap_ || reserve(std::max(bytes, cap_ * 3 / 2)); }
    void reset() {
        if (p_) (void)(pinned_ ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
    }
    size_t cap() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }
    template <class T = void> T* as() const { return static_cast<T*>(p_); }

  protected:
    explicit Buf(bool pinned) : pinned_(pinned) {}

  private:
    bool pinned_;
    void* p_ = nullptr;
    size_t cap_ = 0;
};
struct DeviceBuf : Buf { DeviceBuf() : Buf(false) {} };
struct PinnedBuf : Buf { PinnedBuf() : Buf(true) {} };

}  // namespace pgh_detail
