// hip_handles.h -- owning handles for HIP device / pinned buffers, streams and events (host code only).
//
// One policy for every buffer the engine and the plugin keep between calls: grow only; free the old block before
// allocating the new one (the two never coexist); a failed allocation leaves an empty buffer, never a recorded capacity
// without memory behind it.  reserve() copies nothing, clears nothing and waits for nothing: what may still use the old
// block is the caller's to wait for, before the call.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>

namespace valign {

inline void hip_check(hipError_t e, const char *what) {
    if (e != hipSuccess)
        throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// a failed `call`, named "call(what)" in the error (or just "call")
inline void hip_check_named(hipError_t e, const char *call, const char *what) {
    if (e != hipSuccess) hip_check(e, what ? (std::string(call) + "(" + what + ")").c_str() : call);
}

// PINNED: page-locked host memory (hipHostMallocDefault: mapped, so the device may address it, Engine::dev_view)
template <class T, bool PINNED>
class HipBuffer {
public:
    HipBuffer() = default;
    HipBuffer(HipBuffer &&o) noexcept : p_(o.p_), bytes_(o.bytes_) {
        o.p_ = nullptr;
        o.bytes_ = 0;
    }
    HipBuffer &operator=(HipBuffer &&o) noexcept {
        if (this != &o) {
            reset();
            std::swap(p_, o.p_);
            std::swap(bytes_, o.bytes_);
        }
        return *this;
    }
    ~HipBuffer() { reset(); }

    T *get() const { return p_; }
    size_t bytes() const { return bytes_; }

    void reset() {
        if (p_) (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        bytes_ = 0;
    }

    // at least `bytes` bytes; `what` names the allocation in the error
    void reserve(size_t bytes, const char *what = nullptr) {
        if (bytes <= bytes_) return;
        reset();
        void *p = nullptr;
        hip_check_named(PINNED ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes),
                        PINNED ? "hipHostMalloc" : "hipMalloc", what);
        p_ = static_cast<T *>(p);
        bytes_ = bytes;
    }

private:
    T *p_ = nullptr;
    size_t bytes_ = 0;
};
template <class T>
using DeviceBuffer = HipBuffer<T, false>;
template <class T>
using PinnedBuffer = HipBuffer<T, true>;

struct StreamDestroy {
    void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); }
};
struct EventDestroy {
    void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
};
using StreamHandle = std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamDestroy>;
using EventHandle = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDestroy>;

inline StreamHandle make_stream(const char *what = nullptr) {         // non-blocking: no implicit sync with the null stream
    hipStream_t s = nullptr;
    hip_check_named(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate", what);
    return StreamHandle(s);
}

inline EventHandle make_event(unsigned flags) {
    hipEvent_t e = nullptr;
    hip_check(hipEventCreateWithFlags(&e, flags), "hipEventCreate");
    return EventHandle(e);
}

}  // namespace valign
