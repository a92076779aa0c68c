// ezrs_host.hpp -- host-side plumbing shared by the C ABI files (ezrs_capi.hip, ezbch.hip).
// Host only, header only.  HIP_TRY reports through hip_fail(hipError_t, const char *), which each
// including file defines over its own thread-local error string (ezrs_last_error and
// ezbch_last_error stay separate).
#pragma once

#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstddef>
#include <string>

namespace ezrs {

// Makes `dev` the calling thread's device for a scope.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// Records "<what>: <HIP's text>" in `err` and maps the HIP error to a negative errno.
inline int hip_fail(std::string &err, hipError_t e, const char *what) {
    err = std::string(what) + ": " + hipGetErrorString(e);
    if (e == hipErrorOutOfMemory) return -ENOMEM;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return -ENODEV;
    return -EIO;
}

#define HIP_TRY(expr)                                          \
    do {                                                       \
        hipError_t e_ = (expr);                                \
        if (e_ != hipSuccess) return hip_fail(e_, #expr);      \
    } while (0)

inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// N staging buffers of one size that only grow: device memory (HostFlags < 0) or pinned host memory
// from hipHostMalloc(HostFlags).  Growing frees all N before it allocates any (the peak stays at
// the new size) and keeps no contents; after a failed allocation the size reads 0.
template <int N, int HostFlags = -1>
struct StageBufs {
    void *p[N] = {};
    size_t bytes = 0;             // of each buffer

    hipError_t ensure(size_t need) {
        if (bytes >= need) return hipSuccess;
        release();
        for (int i = 0; i < N; ++i) {
            hipError_t e = HostFlags < 0 ? hipMalloc(&p[i], need)
                                         : hipHostMalloc(&p[i], need, (unsigned)HostFlags);
            if (e != hipSuccess) return e;
        }
        bytes = need;
        return hipSuccess;
    }
    void release() {
        for (int i = 0; i < N; ++i) {
            if (p[i]) (void)(HostFlags < 0 ? hipFree(p[i]) : hipHostFree(p[i]));
            p[i] = nullptr;
        }
        bytes = 0;
    }
};

} // namespace ezrs
