// csrc/spg_hip_buffers.hpp — owners of the three kinds of memory the HIP host code keeps: device memory, fine-grained
// device memory the host writes through the PCIe BAR, and pinned host memory mapped into the device's address space.
// Each frees what it holds when it goes; when to grow, and what has to be idle before a free, is the caller's business.
#pragma once
#include <cstring>
#include <hip/hip_runtime.h>

#pragma GCC visibility push(hidden)   // (inline members: not symbols of the library)
namespace spg {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;      // bytes, where the owner allocates through alloc() / alloc_fine()
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t release() {
        const hipError_t e = p ? hipFree(p) : hipSuccess;
        p = nullptr; cap = 0;
        return e;
    }
    hipError_t alloc(size_t bytes) { return took(hipMalloc(&p, bytes), bytes); }
    // fine-grained: host stores through the BAR become visible to a running kernel (may be refused: not every system has it)
    hipError_t alloc_fine(size_t bytes) { return took(hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained), bytes); }

private:
    hipError_t took(hipError_t e, size_t bytes) {
        if (e == hipSuccess) cap = bytes; else { p = nullptr; cap = 0; }
        return e;
    }
};

// Pinned host memory and its address on the device. A fresh block is zero-filled (a fresh mailbox never looks ready).
struct PinnedBuf {
    void *h = nullptr, *d = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { if (h) (void)hipHostFree(h); }
    hipError_t release() {
        const hipError_t e = h ? hipHostFree(h) : hipSuccess;
        h = d = nullptr; cap = 0;
        return e;
    }
    hipError_t alloc(size_t bytes) {
        hipError_t e = hipHostMalloc(&h, bytes, hipHostMallocMapped);
        if (e != hipSuccess) { h = nullptr; return e; }
        if ((e = hipHostGetDevicePointer(&d, h, 0)) != hipSuccess) return e;
        memset(h, 0, bytes);
        cap = bytes;
        return hipSuccess;
    }
};

}  // namespace spg
#pragma GCC visibility pop
