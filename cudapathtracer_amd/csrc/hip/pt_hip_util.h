// pt_hip_util.h -- what the library's host code over the HIP runtime shares: the error check, device buffers
// grown or uploaded, and a device allocation that lives for one scope.  Host only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

#include "../host/host_internal.h"

// A HIP call that must succeed: on an error the enclosing function returns PT_E_HIP with the call's text and the
// runtime's message.
#define HIP_TRY(call)                                                                                      \
    do {                                                                                                   \
        const hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) return pt::fail(PT_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_));    \
    } while (0)

// (Internal linkage: every translation unit has its own copies, and the library exports none of them.)
namespace pt {
namespace {

// A device buffer grown on demand (*have counts T's): freed and allocated anew when smaller than `need`.
// The slot is null and 0 before the hipMalloc, so a failed grow leaves it consistent.
template <typename T>
int grow(T** buf, size_t* have, size_t need)
{
    if (*have >= need) return PT_OK;
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr;
    *have = 0;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(buf), need * sizeof(T)));
    *have = need;
    return PT_OK;
}

template <typename T>
int upload(T** dst, const std::vector<T>& src)
{
    size_t bytes = src.size() * sizeof(T);
    if (bytes == 0) bytes = sizeof(T);
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(dst), bytes));
    if (!src.empty()) HIP_TRY(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return PT_OK;
}

// A device allocation freed at the end of its scope, on every path out of it.  It stands where a plain T* stood:
// it converts to the pointer, and &d is the T** that hipMalloc fills.
template <typename T>
class ScopedDevice {
public:
    ScopedDevice() = default;
    ScopedDevice(const ScopedDevice&) = delete;
    ScopedDevice& operator=(const ScopedDevice&) = delete;
    ~ScopedDevice() { if (p_) (void)hipFree(p_); }
    operator T*() const { return p_; }
    T** operator&() { return &p_; }

private:
    T* p_ = nullptr;
};

}  // namespace
}  // namespace pt
