// ceg_grid_common.h -- what the entry points of the site extraction share on the host side (ceg_grid_sites.hip, ceg_grid_coalesce.hip): the error
// return, the device guard, the stream-ordered workspace of one call, the argument checks, and the one load of a map element.
#ifndef CEG_GRID_COMMON_H
#define CEG_GRID_COMMON_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <limits>
#include <vector>

#include "../../include/ceg_hip.h"

extern "C" void ceg_set_last_error_(const char* msg);

namespace ceg_gs {

inline int gerr(int code, const char* msg)
{
    ceg_set_last_error_(msg);
    return code;
}

// a map element as every stage sees it: an FP64 value, or scale * bin with one rounding
__device__ __forceinline__ double gs_load(const double* p, int64_t x, double, int32_t*) { return p[x]; }

__device__ __forceinline__ double gs_load(const int64_t* p, int64_t x, double scale, int32_t* bad)
{
    const int64_t v = p[x];
    if (v >= (1ll << 53) || v <= -(1ll << 53)) *bad = 1;            // the same value from whoever sees one
    return scale * (double)v;                                       // the conversion is exact: one rounding
}

struct DevGuard {
    int prev = -1;
    bool ok = false;
    explicit DevGuard(int d)
    {
        (void)hipGetDevice(&prev);
        ok = hipSetDevice(d) == hipSuccess;
    }
    ~DevGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// stream-ordered workspace of one call: everything it handed out is freed behind the call's last launch
struct Workspace {
    hipStream_t st;
    std::vector<void*> held;
    bool failed = false;
    bool staged = false;          // an input came from host memory: the call synchronises before it returns
    explicit Workspace(hipStream_t s) : st(s) {}
    ~Workspace()
    {
        for (void* p : held) (void)hipFreeAsync(p, st);
    }
    void* get(size_t bytes)
    {
        void* p = nullptr;
        if (hipMallocAsync(&p, bytes ? bytes : 1, st) != hipSuccess) {
            failed = true;
            return nullptr;
        }
        held.push_back(p);
        return p;
    }
    const void* in(const void* src, int on_device, size_t bytes)
    {
        if (on_device) return src;
        staged = true;
        void* p = get(bytes);
        if (p && bytes && hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess) failed = true;
        return p;
    }
    void* out(void* dst, int on_device, size_t bytes) { return (on_device || !dst) ? dst : get(bytes); }
    void back(void* dst, int on_device, const void* dev, size_t bytes)
    {
        if (dst && !on_device && bytes && hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToHost, st) != hipSuccess) failed = true;
    }
};

inline int check_dims(const int32_t* dims, int64_t* n)
{
    if (!dims || dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return gerr(CEG_ERR_INVALID, "dims must be three positive numbers");
    const int64_t ab = (int64_t)dims[0] * dims[1];
    if (ab > std::numeric_limits<int32_t>::max() || ab * dims[2] > std::numeric_limits<int32_t>::max())
        return gerr(CEG_ERR_INVALID, "a*b*c does not fit int32");
    *n = ab * dims[2];
    return CEG_OK;
}

inline int check_device(int32_t device)
{
    if (ceg_device_count() <= 0) return gerr(CEG_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ceg_device_count()) return gerr(CEG_ERR_NO_DEVICE, "device not present");
    return CEG_OK;
}

}  // namespace ceg_gs

#endif  // CEG_GRID_COMMON_H
