// afx_hipcheck.h -- error-check macros and launch helpers shared by the .hip translation units
#ifndef AFX_HIPCHECK_H
#define AFX_HIPCHECK_H

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <mutex>

#include "afx_device.h"

#define AFX_HIP(call)                                                                      \
    do {                                                                                   \
        hipError_t _e = (call);                                                            \
        if (_e != hipSuccess) {                                                            \
            afxdev_set_error("%s failed at %s:%d: %s", #call, __FILE__, __LINE__,          \
                             hipGetErrorString(_e));                                       \
            return AFX_ERR_HIP;                                                            \
        }                                                                                  \
    } while (0)

// after a kernel launch
#define AFX_LAUNCH_CHECK(name)                                                             \
    do {                                                                                   \
        hipError_t _e = hipGetLastError();                                                 \
        if (_e != hipSuccess) {                                                            \
            afxdev_set_error("launch of %s failed: %s", name, hipGetErrorString(_e));      \
            return AFX_ERR_HIP;                                                            \
        }                                                                                  \
    } while (0)

// CUs of the current device, queried per launch (256 when the query fails)
static inline int afx_cu_count() {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return cus;
}

// Raises the dynamic-LDS limit of kernel K to `bytes` before its first launch on a device.  One latch per kernel
// instantiation and device (the attribute lives in the device's code object); two threads may both set it: idempotent.
template <auto K>
int afx_dyn_lds(int bytes) {
    static std::atomic<bool> attrSet[AFX_MAX_DEVICES];
    const int dev = afxdev_current_device() & (AFX_MAX_DEVICES - 1);
    if (!attrSet[dev].load(std::memory_order_acquire)) {
        AFX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(K), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        attrSet[dev].store(true, std::memory_order_release);
    }
    return AFX_OK;
}

// Launch of a kernel instantiation that needs more dynamic LDS than the default limit; `kernel` in parentheses when its
// template argument list has commas.  Returns AFX_ERR_HIP from the calling function when the attribute cannot be set.
#define AFX_LAUNCH_DYN_LDS(kernel, grid, block, lds, stream, ...)                              \
    do {                                                                                       \
        if (const int st_ = afx_dyn_lds<kernel>((int)(lds))) return st_;                       \
        hipLaunchKernelGGL(kernel, grid, block, lds, (hipStream_t)(stream), __VA_ARGS__);      \
    } while (0)

// A constant table (twiddles) that FILL writes into `bytes` zeroed host bytes: one device copy per device, built on first
// use, never freed; nullptr when it cannot be had.  The copy is synchronous: the caller's stream is not waited for under
// the lock.  One cache per FILL.
template <void (*FILL)(float *)>
const float *afx_device_table(size_t bytes) {
    static std::mutex mu;
    static float *dTab[AFX_MAX_DEVICES] = {};
    const int dev = afxdev_current_device();
    if (dev < 0 || dev >= AFX_MAX_DEVICES) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    if (!dTab[dev]) {
        float *h = static_cast<float *>(calloc(bytes, 1));
        if (!h) return nullptr;
        FILL(h);
        float *d = nullptr;
        int st = afxdev_malloc(reinterpret_cast<void **>(&d), bytes);
        if (st == AFX_OK && hipMemcpy(d, h, bytes, hipMemcpyHostToDevice) != hipSuccess) st = AFX_ERR_HIP;
        free(h);
        if (st != AFX_OK) {
            afxdev_free(d);
            return nullptr;
        }
        dTab[dev] = d;
    }
    return dTab[dev];
}

#endif
