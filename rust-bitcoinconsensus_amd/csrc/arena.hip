// The grow-only device and page-locked buffers of arena.h.
#include "arena.h"
#include "gpu_common.h"

namespace bcc {

int DeviceBuf::release() {
    if (p) BCC_HIP_TRY(hipFree(p));
    p = nullptr;
    cap = 0;
    return 0;
}

int DeviceBuf::reserve(size_t bytes) {
    if (bytes <= cap) return 0;
    if (int e = release()) return e;
    BCC_HIP_TRY(hipMalloc(&p, bytes));
    cap = bytes;
    return 0;
}

DeviceBuf::~DeviceBuf() {
    if (p) (void)hipFree(p);
}

int PinnedBuf::release() {
    if (p) BCC_HIP_TRY(hipHostFree(p));
    p = nullptr;
    dev = nullptr;
    cap = 0;
    return 0;
}

int PinnedBuf::grow(size_t bytes, bool mapped) {
    if (bytes <= cap) return 0;
    if (int e = release()) return e;
    BCC_HIP_TRY(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    if (mapped) BCC_HIP_TRY(hipHostGetDevicePointer(&dev, p, 0));
    cap = bytes;
    return 0;
}

PinnedBuf::~PinnedBuf() {
    if (p) (void)hipHostFree(p);
}

}  // namespace bcc
