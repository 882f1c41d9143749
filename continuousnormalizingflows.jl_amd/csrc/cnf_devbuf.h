// cnf_devbuf.h — the one place of the host layer that allocates and frees: a move-only owner of one hipMalloc allocation
// (DevBuf<T>) or one block of pinned host memory (PinnedBuf<T>).  Host code only.
#pragma once
#include <cstddef>
#include <utility>

#include <hip/hip_runtime.h>

namespace cnf {

// Grow-only: reserve(count) on a buffer that already holds `count` elements makes no HIP call.  No zero-fill, no rounding, no
// pooling: a caller that wants its capacity rounded rounds `count` itself.  The device that is current when the buffer is
// released (or destroyed) must be the one it was allocated on.
template <class T, bool Pinned = false>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p_ = std::exchange(o.p_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    ~DevBuf() { release(); }

    // At least `count` elements.  Growing frees the old allocation first (its contents are not kept); a failed allocation leaves
    // the buffer empty (null, capacity 0).  `grew` (may be null) reports whether the allocation was replaced.
    hipError_t reserve(size_t count, bool* grew = nullptr) {
        if (grew) *grew = false;
        if (count <= cap_) return hipSuccess;
        if (grew) *grew = true;
        if (p_) {
            const hipError_t e = free_(p_);
            if (e != hipSuccess) return e;
        }
        p_ = nullptr;
        cap_ = 0;
        void* q = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&q, count * sizeof(T), hipHostMallocDefault) : hipMalloc(&q, count * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(q);
        cap_ = count;
        return hipSuccess;
    }
    void release() {
        if (p_) (void)free_(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    T* data() const { return p_; }
    operator T*() const { return p_; }
    size_t capacity() const { return cap_; }   // elements

private:
    static hipError_t free_(T* p) { return Pinned ? hipHostFree(p) : hipFree(p); }
    T* p_ = nullptr;
    size_t cap_ = 0;
};

template <class T>
using PinnedBuf = DevBuf<T, true>;

}  // namespace cnf
