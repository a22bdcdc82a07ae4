// ceg_host.h -- host-side helpers that the translation units of libceg_hip.so share (namespace ceg_host).  Nothing here reaches
// device code: what the kernels see is ceg_internal.h.  Defined in ceg_api.hip unless noted.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ceg_hip.h"

namespace ceg_host {

// sets the calling thread's ceg_last_error() text (printf format) and returns `code`
int fail(int code, const char* fmt, ...);

// the argument checks every plan creation and one-shot entry point starts with
int check_common(const double* pos, int64_t natoms, const double* mat, const double* invmat,
                 const int32_t* dims, const double* size, const double* shift, const double* delta);

// the plan-table block cache (small device arrays by power-of-two size class)
hipError_t pool_malloc(void** out, size_t bytes);
void pool_free(void* ptr);

// frees the idle page-locked buffers, device slabs and stream pairs of the one-shot pools (ceg_oneshot.hip); called by
// ceg_release_cached_buffers
void oneshot_pools_release();

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = (hipSetDevice(dev) == hipSuccess);
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

}  // namespace ceg_host

#define HIP_TRY(expr)                                                                                \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return ceg_host::fail(CEG_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                  __FILE__, __LINE__);                                               \
    } while (0)
