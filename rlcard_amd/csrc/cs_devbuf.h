// cs_devbuf.h -- host-side device-memory helpers of the ABI layer and the launchers (no kernels): a device buffer that
// grows on demand, and the carver of one allocation into 256-B-aligned parts.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace cs {

// A device allocation grown on demand; reserve never shrinks it, and a failed reserve leaves it empty.
// The old block goes back through plain hipFree on purpose: hipFree synchronises the device, which is what makes it
// safe to free a buffer that an earlier launch on any stream may still read. (An async free would not be.)
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;

    hipError_t reserve(size_t need)
    {
        if (need <= bytes) return hipSuccess;
        release();
        const hipError_t e = hipMalloc(&p, need);
        if (e != hipSuccess) p = nullptr;
        else bytes = need;
        return e;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// Offsets of the parts of one allocation, in the order taken, each part starting 256-B aligned (so take<T>(1) is a
// 256-B block of its own); bytes() is the size so far, a multiple of 256.
struct Carve {
    size_t total = 0;

    template <class T>
    size_t take(size_t count)
    {
        const size_t o = total;
        total += (count * sizeof(T) + 255) / 256 * 256;
        return o;
    }
    size_t bytes() const { return total; }
};

}  // namespace cs
