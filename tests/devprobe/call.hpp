// call.hpp -- what every device probe of this library shares (probe.hip, gp_probe.hip): the guard bytes and the sentinel
// behind every output buffer, the refusal codes, and the device buffers of one probe call.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <vector>

namespace {

constexpr int kPad = 256;                  // guard bytes behind every output buffer
constexpr int kFill = 0xA5;                // sentinel byte
constexpr int kMaxBlocks = 64;             // workgroups of one launch
constexpr int kBadShape = -1, kBadSize = -2;

// device buffers of one probe call
struct Call {
    struct Out { void* dev; void* host; size_t bytes; };
    std::vector<void*> owned;
    std::vector<Out> outs;
    hipError_t err = hipSuccess;

    void* alloc(size_t bytes) {
        void* p = nullptr;
        if (err == hipSuccess) err = hipMalloc(&p, bytes ? bytes : 8);
        if (err != hipSuccess) return nullptr;
        owned.push_back(p);
        return p;
    }
    template <class T>
    const T* in(const T* host, size_t count) {
        void* p = alloc(count * sizeof(T));
        if (p && count) err = hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice);
        return (const T*)p;
    }
    // `host` has room for count elements plus kPad bytes
    template <class T>
    T* out(T* host, size_t count) {
        const size_t bytes = count * sizeof(T) + kPad;
        void* p = alloc(bytes);
        if (p) err = hipMemset(p, kFill, bytes);
        if (p) outs.push_back({p, host, bytes});
        return (T*)p;
    }
    bool ok() const { return err == hipSuccess; }
    int finish() {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
        for (const Out& o : outs)
            if (err == hipSuccess) err = hipMemcpy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost);
        for (void* p : owned) (void)hipFree(p);
        return (int)err;
    }
};

}  // namespace
