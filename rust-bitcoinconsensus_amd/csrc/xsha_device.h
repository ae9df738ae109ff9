// The streaming SHA-256 slot of the extraction kernels (sighash.hip K_win / K_lin / the Taproot
// kernels, block_hash.hip K_txh): every lane streams bytes into a SHA-256 whose 64-byte block
// buffer and state live in the lane's own LDS slot (96 bytes, + 4 so that lane slots start on
// different banks), so byte positions can be dynamic without scratch memory; the compression
// reads the block back as 16 words.  Device code only: included by the .hip files that own such
// kernels, each of which declares `lds[XS_WG * XS_SLOT]`.
#pragma once
#include "gpu_common.h"
#include "sha256_device.h"

namespace bcc {

__device__ __forceinline__ uint32_t bswap_u32(uint32_t x) { return __builtin_bswap32(x); }

constexpr int XS_SLOT = 100;   // bytes per lane: block[64] | state[32] | pad

__device__ __noinline__ void xs_compress(uint8_t* slot) {
    const uint32_t* b = reinterpret_cast<const uint32_t*>(slot);
    uint32_t* st = reinterpret_cast<uint32_t*>(slot + 64);
    uint32_t w[16], s8[8];
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = bswap_u32(b[k]);
#pragma unroll
    for (int k = 0; k < 8; k++) s8[k] = st[k];
    sha256_compress(s8, w);
#pragma unroll
    for (int k = 0; k < 8; k++) st[k] = s8[k];
}

struct XSha {
    uint8_t* slot;
    uint32_t fill;   // bytes in the block buffer
    uint32_t total;  // message bytes so far
};

__device__ __forceinline__ void xs_init(XSha& h, uint8_t* slot) {
    h.slot = slot;
    h.fill = 0;
    h.total = 0;
    uint32_t* st = reinterpret_cast<uint32_t*>(slot + 64);
    uint32_t iv[8];
    sha256_init_state(iv);
#pragma unroll
    for (int k = 0; k < 8; k++) st[k] = iv[k];
}

// n message bytes from global memory.  Per step: the (up to 17) aligned dwords covering the next
// min(n, 64 - fill) source bytes are loaded together (one memory latency per block, not per
// byte), realigned with funnel shifts, and written into the block buffer: as dwords when the fill
// position is 4-aligned, else byte by byte.  Bytes written past the step's end are scratch that a
// later step or the padding overwrites (the slot has 4 spare bytes after the block).
__device__ __forceinline__ void xs_put(XSha& h, const uint8_t* __restrict__ src, uint32_t n) {
    h.total += n;
    while (n) {
        const uint32_t take = min(n, 64u - h.fill);
        const uintptr_t a = reinterpret_cast<uintptr_t>(src);
        const uint32_t* w = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
        const uint32_t sh = (uint32_t)(a & 3), nd = (sh + take + 3) >> 2;
        uint32_t v[17];
#pragma unroll
        for (int k = 0; k < 17; k++) v[k] = (uint32_t)k < nd ? w[k] : 0u;
        uint32_t r[16];
#pragma unroll
        for (int k = 0; k < 16; k++) r[k] = __builtin_amdgcn_alignbyte(v[k + 1], v[k], sh);
        uint8_t* dst = h.slot + h.fill;
        if ((h.fill & 3) == 0) {
            uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
            for (int k = 0; k < 16; k++)
                if ((uint32_t)(4 * k) < take) d4[k] = r[k];
        } else {
#pragma unroll
            for (int i = 0; i < 64; i++)
                if ((uint32_t)i < take) dst[i] = (uint8_t)(r[i >> 2] >> (8 * (i & 3)));
        }
        h.fill += take;
        src += take;
        n -= take;
        if (h.fill == 64) {
            xs_compress(h.slot);
            h.fill = 0;
        }
    }
}

// SHA-256 padding + final compression(s), then the second SHA-256 of SHA-256d: the digest as
// eight big-endian words.
__device__ __forceinline__ void xs_final_dw(XSha& h, uint32_t e[8]) {
    const uint64_t bits = (uint64_t)h.total * 8;
    h.slot[h.fill++] = 0x80;
    if (h.fill > 56) {
        while (h.fill < 64) h.slot[h.fill++] = 0;
        xs_compress(h.slot);
        h.fill = 0;
    }
    while (h.fill < 56) h.slot[h.fill++] = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) h.slot[56 + k] = (uint8_t)(bits >> (8 * (7 - k)));
    xs_compress(h.slot);
    const uint32_t* st = reinterpret_cast<const uint32_t*>(h.slot + 64);
    uint32_t d[8];
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = st[k];
    sha256_of_digest(e, d);
}

// ... as big-endian digest bytes to out (16-aligned).
__device__ __forceinline__ void xs_final_d(XSha& h, uint8_t* __restrict__ out) {
    uint32_t e[8];
    xs_final_dw(h, e);
    uint4* o = reinterpret_cast<uint4*>(out);
    o[0] = make_uint4(bswap_u32(e[0]), bswap_u32(e[1]), bswap_u32(e[2]), bswap_u32(e[3]));
    o[1] = make_uint4(bswap_u32(e[4]), bswap_u32(e[5]), bswap_u32(e[6]), bswap_u32(e[7]));
}

// the first `n` (<= 4) little-endian bytes of v, from registers
__device__ __forceinline__ void xs_put_le(XSha& h, uint32_t v, uint32_t n) {
    h.total += n;
    for (uint32_t k = 0; k < n; k++) {
        h.slot[h.fill++] = (uint8_t)(v >> (8 * k));
        if (h.fill == 64) {
            xs_compress(h.slot);
            h.fill = 0;
        }
    }
}

// xs_put behind a dword-aligned fill: the (at most three) bytes up to the next dword boundary of
// the block buffer go in from registers first, so that xs_put takes its dword path.  K_lin's 41-byte
// input records leave the fill unaligned three times out of four, and a wave takes xs_put's
// byte-by-byte path when any of its lanes does.
__device__ __forceinline__ void xs_put_headed(XSha& h, const uint8_t* __restrict__ src, uint32_t n) {
    const uint32_t head = (4u - (h.fill & 3u)) & 3u;
    if (head && n > head) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(src);
        const uint32_t* w = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
        const uint32_t sh = (uint32_t)(a & 3);
        const uint32_t lo = w[0], hi = sh + head > 4u ? w[1] : 0u;  // (only the dwords the bytes are in)
        xs_put_le(h, __builtin_amdgcn_alignbyte(hi, lo, sh), head);
        src += head;
        n -= head;
    }
    xs_put(h, src, n);
}

}  // namespace bcc
