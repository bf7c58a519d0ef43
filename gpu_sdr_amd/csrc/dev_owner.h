// dev_owner.h -- move-only owners of what this library creates on the device: a buffer of T, a stream, an event.
// An owner releases what it holds when it is destroyed, reset or assigned to; an empty one makes no HIP call at all.
// They order nothing: whoever destroys a holder first waits for the streams that may still use its buffers
// (gsdr_demod_close, gsdr_txgen_close).  Internal to csrc/; needs only the HIP runtime header, so a host compiler
// builds it alone (tests/test_dev_owner_host.py).
#ifndef GSDR_DEV_OWNER_H
#define GSDR_DEV_OWNER_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

namespace gsdr {

// `count` elements of T in device memory.  Converts to T*, so launch sites read as with a raw pointer.
template <typename T>
class DevBuf {
    T *p_ = nullptr;

  public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) reset(), p_ = o.p_, o.p_ = nullptr;
        return *this;
    }
    ~DevBuf() { reset(); }
    operator T *() const { return p_; }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
    }
    // Each of the three frees what the owner held, and leaves it empty when a step fails.  A count of 0 allocates one element.
    hipError_t alloc(size_t count) {
        reset();
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p_), (count ? count : 1) * sizeof(T));
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    hipError_t alloc_zeroed(size_t count) {
        hipError_t e = alloc(count);
        if (e == hipSuccess && (e = hipMemset(p_, 0, count * sizeof(T))) != hipSuccess) reset();
        return e;
    }
    // an empty vector allocates one element and copies nothing
    hipError_t upload(const std::vector<T> &src) {
        hipError_t e = alloc(src.size());
        if (e == hipSuccess && !src.empty() &&
            (e = hipMemcpy(p_, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice)) != hipSuccess)
            reset();
        return e;
    }
};

// A stream or an event created by this library: `hipEventCreate(e.out())`, then `e` wherever the raw handle goes.
template <typename H, hipError_t (*Destroy)(H)>
class DevHandle {
    H h_ = nullptr;

  public:
    DevHandle() = default;
    DevHandle(DevHandle &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    DevHandle &operator=(DevHandle &&o) noexcept {
        if (this != &o) reset(), h_ = o.h_, o.h_ = nullptr;
        return *this;
    }
    ~DevHandle() { reset(); }
    operator H() const { return h_; }
    void reset() {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }
    // where a create function stores the new handle (what the owner held is destroyed first)
    H *out() {
        reset();
        return &h_;
    }
};
using Stream = DevHandle<hipStream_t, hipStreamDestroy>;
using Event = DevHandle<hipEvent_t, hipEventDestroy>;

}  // namespace gsdr

#endif
