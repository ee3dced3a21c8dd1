// tdoa_devmem.h -- the move-only owner of one hipMalloc that the contexts
// (tdoa_capi.cpp) and the streaming pipelines (tdoa_stream.cpp) hold their
// device memory in, and the HIP error check both use.  Host code only.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>

#include <utility>

#include "../../include/tdoa.h"
#include "tdoa_shared.h"

#define HIP_TRY(expr)                                                               \
    do {                                                                            \
        hipError_t e_ = (expr);                                                     \
        if (e_ != hipSuccess)                                                       \
            return tdoa_fail(TDOA_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

class tdoa_devmem {
public:
    tdoa_devmem() = default;
    tdoa_devmem(const tdoa_devmem &) = delete;
    tdoa_devmem &operator=(const tdoa_devmem &) = delete;
    tdoa_devmem(tdoa_devmem &&o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    tdoa_devmem &operator=(tdoa_devmem &&o) noexcept
    {
        std::swap(p_, o.p_);  // what this held goes with o
        std::swap(bytes_, o.bytes_);
        return *this;
    }
    // the owning context or pipeline selects the device before it is released
    ~tdoa_devmem() { release(); }

    void release()
    {
        if (p_)
            (void)hipFree(p_);
        p_ = nullptr;
        bytes_ = 0;
    }
    // a fresh allocation of `bytes`; holds nothing on failure
    hipError_t alloc(size_t bytes)
    {
        release();
        const hipError_t e = hipMalloc(&p_, bytes);
        if (e != hipSuccess)
            p_ = nullptr;
        else
            bytes_ = bytes;
        return e;
    }
    // copy `bytes` from the host into the allocation (made here if none is held)
    hipError_t upload(const void *host, size_t bytes)
    {
        if (!p_) {
            const hipError_t e = alloc(bytes);
            if (e != hipSuccess)
                return e;
        }
        return hipMemcpy(p_, host, bytes, hipMemcpyHostToDevice);
    }
    // scratch that grows on demand: synchronises the stream before a resize
    int grow(size_t need, void *stream, const char *what)
    {
        if (need <= bytes_)
            return TDOA_OK;
        HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
        if (alloc(need) != hipSuccess)
            return tdoa_fail(TDOA_ERR_NOMEM, "%s scratch of %zu bytes", what, need);
        return TDOA_OK;
    }
    template <typename T> T *get() const { return static_cast<T *>(p_); }
    size_t bytes() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    void *p_ = nullptr;
    size_t bytes_ = 0;
};
