// Device arenas: one layout rule and the two grow-only buffers every staging site uses.
// An arena is a run of regions, each starting on a 256-byte boundary; a site keeps an enum-indexed
// sizes[] table and takes the offsets from arena_layout.  The buffers (arena.hip) never keep their
// contents across a reserve and never round what the caller asks for.  No HIP header here: the
// host code and the CPU test builds include this through pipeline.h.
#pragma once
#include <cstddef>
#include <cstdint>

namespace bcc {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// off[i + 1] = off[i] + align256(sizes[i]) from off[0] = 0; returns off[nb], the arena's bytes.
// A zero-size region takes no bytes (off[i + 1] == off[i]).
inline size_t arena_layout(const size_t* sizes, size_t* off, int nb) {
    off[0] = 0;
    for (int i = 0; i < nb; i++) off[i + 1] = off[i] + align256(sizes[i]);
    return off[nb];
}

// reserve(bytes): nothing when bytes <= cap; else the old block is freed, the buffer is empty, and
// exactly `bytes` are allocated.  Returns 0 or the hipError_t of the failing call: a failed free
// leaves the buffer as it was, a failed allocation leaves it empty.  The caller makes the owning
// device current before reserve, release and destruction.
struct DeviceBuf {
    void* p = nullptr;
    size_t cap = 0;
    DeviceBuf() = default;
    DeviceBuf(DeviceBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DeviceBuf(const DeviceBuf&) = delete;
    DeviceBuf& operator=(const DeviceBuf&) = delete;
    ~DeviceBuf();
    int reserve(size_t bytes);
    int release();
    uint8_t* bytes() const { return (uint8_t*)p; }
};

// The same in page-locked host memory.  reserve_mapped also takes the block's device-side address
// (hipHostGetDevicePointer) into `dev`, for the verdict buffers a kernel writes; cap counts only
// once that succeeded.
struct PinnedBuf {
    void* p = nullptr;
    void* dev = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf();
    int reserve(size_t bytes) { return grow(bytes, false); }
    int reserve_mapped(size_t bytes) { return grow(bytes, true); }
    int release();
    uint8_t* bytes() const { return (uint8_t*)p; }

private:
    int grow(size_t bytes, bool mapped);
};

}  // namespace bcc
