// Block header chains: what one round carries between the host pass (host/headers.cpp) and the
// device (header_check.hip), and the lane code both run.  No HIP header here: csrc/host and the
// CPU test builds include this.
//
//   hash        = SHA-256d of the 80 header bytes (primitives/block.cpp GetHash)
//   proof of work: CheckProofOfWork (pow.cpp:74-91) over arith_uint256::SetCompact
//                 (arith_uint256.cpp:203-221)
//   context     : ContextualCheckBlockHeader (validation.cpp:3496-3535) with GetNextWorkRequired /
//                 CalculateNextWorkRequired (pow.cpp:13-72), GetCompact (arith_uint256.cpp:223-244)
//                 and GetMedianTimePast (chain.h:257-275)
// 256-bit numbers are eight 32-bit limbs, limb 0 the least significant: a hash row read as
// little-endian words is the arith_uint256 of that hash.  Nothing below indexes a limb array with
// a value the compiler cannot see, so the device keeps them in registers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "bcc_amd.h"
#include "block_hash.h"

namespace bcc {

constexpr uint32_t HEADER_BYTES = 80, HEADER_WORDS = 20, MTP_SPAN = 11;
// words of a header: nVersion, hashPrevBlock[8], hashMerkleRoot[8], nTime, nBits, nNonce
enum { HW_VERSION = 0, HW_PREV = 1, HW_TIME = 17, HW_BITS = 18 };

// The consensus parameters and what the round's lanes need from before its first header
// (host/headers.cpp header_context_at is the one place that fills the second half).
struct HeaderRoundCtx {
    uint32_t pow_limit[8];
    int64_t timespan;  // nPowTargetTimespan: 4 * timespan fits 32 bits
    int64_t max_time;  // 0: the time-too-new rule is off
    uint32_t interval;
    uint32_t no_retarget;
    int32_t bip34, bip66, bip65;
    int32_t height0;    // height of the round's header 0
    uint32_t genesis0;  // the round's header 0 is a genesis: the proof of work only
    uint32_t prev_bits;
    uint32_t prev_hash[8];
    uint32_t times[MTP_SPAN];  // nTime of the blocks before header 0, newest first
    uint32_t n_times;
    uint32_t period_first_time;  // nTime of the block `interval` below the first retarget
                                 // boundary at or above height0, when that block is before the round
};

// Word k of the header bytes at p.  The device's arena is aligned; the host reads the caller's
// bytes wherever they are.
SHA_HD uint32_t hdr_word(const uint8_t* p, size_t k) {
#if defined(__HIP_DEVICE_COMPILE__)
    return reinterpret_cast<const uint32_t*>(p)[k];
#else
    uint32_t v;
    memcpy(&v, p + 4 * k, 4);
    return v;
#endif
}

// SHA-256d of a header given as its 20 little-endian words; out: the digest as the words of the
// raw hash row (= the limbs of its arith_uint256).
SHA_HD void header_hash_lane(const uint32_t (&h)[HEADER_WORDS], uint32_t (&out)[8]) {
    uint32_t s[8], w[16], d[8];
#pragma unroll
    for (int j = 0; j < 16; j++) w[j] = merkle_bswap(h[j]);
    sha256_init_state(s);
    sha256_compress(s, w);
#pragma unroll
    for (int j = 0; j < 4; j++) w[j] = merkle_bswap(h[16 + j]);
    w[4] = 0x80000000u;
#pragma unroll
    for (int j = 5; j < 15; j++) w[j] = 0;
    w[15] = HEADER_BYTES * 8;
    sha256_compress(s, w);
    sha256_of_digest(d, s);
#pragma unroll
    for (int j = 0; j < 8; j++) out[j] = merkle_bswap(d[j]);
}

SHA_HD bool u256_gt(const uint32_t (&a)[8], const uint32_t (&b)[8]) {
    bool gt = false, decided = false;
#pragma unroll
    for (int j = 7; j >= 0; j--) {
        if (!decided && a[j] != b[j]) {
            gt = a[j] > b[j];
            decided = true;
        }
    }
    return gt;
}
SHA_HD bool u256_zero(const uint32_t (&a)[8]) {
    uint32_t o = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) o |= a[j];
    return o == 0;
}
// limb k of a, zero for k >= 8
SHA_HD uint32_t u256_limb(const uint32_t (&a)[8], uint32_t k) {
    uint32_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) v = j == k ? a[j] : v;
    return v;
}

// SetCompact: t = the target; returns COMPACT_NEGATIVE / COMPACT_OVERFLOW.  A shift past 256 bits
// drops the mantissa, as base_uint::operator<<= does.
enum : uint32_t { COMPACT_NEGATIVE = 1, COMPACT_OVERFLOW = 2 };
SHA_HD uint32_t compact_expand(uint32_t bits, uint32_t (&t)[8]) {
    const uint32_t size = bits >> 24;
    uint32_t word = bits & 0x007fffffu;
    uint32_t limb = 0, lo, hi = 0;
    if (size <= 3) {
        word >>= 8 * (3 - size);
        lo = word;
    } else {
        const uint32_t sh = 8 * (size - 3);
        const uint32_t b = sh & 31u;
        limb = sh >> 5;
        lo = word << b;
        hi = b ? word >> (32 - b) : 0u;
    }
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) t[j] = (j == limb ? lo : 0u) | (j == limb + 1 ? hi : 0u);
    uint32_t f = 0;
    if (word != 0 && (bits & 0x00800000u)) f |= COMPACT_NEGATIVE;
    if (word != 0 && (size > 34 || (word > 0xffu && size > 33) || (word > 0xffffu && size > 32)))
        f |= COMPACT_OVERFLOW;
    return f;
}

// GetCompact(false), the sign-bit renormalisation included.
SHA_HD uint32_t compact_get(const uint32_t (&t)[8]) {
    uint32_t nbits = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++)
        if (t[j]) nbits = 32 * j + 32 - (uint32_t)__builtin_clz(t[j]);
    uint32_t size = (nbits + 7) / 8, c;
    if (size <= 3) {
        c = t[0] << (8 * (3 - size));
    } else {
        const uint32_t sh = 8 * (size - 3), b = sh & 31u, limb = sh >> 5;
        const uint32_t lo = u256_limb(t, limb), hi = u256_limb(t, limb + 1);
        c = (lo >> b) | (b ? hi << (32 - b) : 0u);
    }
    if (c & 0x00800000u) {
        c >>= 8;
        size++;
    }
    return c | (size << 24);
}

// CheckProofOfWork(hash, bits) under pow_limit.
SHA_HD bool pow_check(const uint32_t (&hash)[8], uint32_t bits, const uint32_t (&limit)[8]) {
    uint32_t t[8];
    const uint32_t f = compact_expand(bits, t);
    if (f || u256_zero(t) || u256_gt(t, limit)) return false;
    return !u256_gt(hash, t);
}

// CalculateNextWorkRequired: the bits after a period whose last block has last_bits / last_time
// and whose first block has first_time.  The product keeps its low 256 bits, as
// base_uint::operator*=(uint32_t) does.
SHA_HD uint32_t next_work_required(uint32_t last_bits, uint32_t last_time, uint32_t first_time,
                                   const HeaderRoundCtx& c) {
    if (c.no_retarget) return last_bits;
    int64_t span = (int64_t)last_time - (int64_t)first_time;
    if (span < c.timespan / 4) span = c.timespan / 4;
    if (span > c.timespan * 4) span = c.timespan * 4;
    uint32_t t[8];
    compact_expand(last_bits, t);
    const uint32_t m = (uint32_t)span, d = (uint32_t)c.timespan;
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint64_t p = carry + (uint64_t)m * t[j];
        t[j] = (uint32_t)p;
        carry = p >> 32;
    }
    uint64_t rem = 0;
#pragma unroll
    for (int j = 7; j >= 0; j--) {
        const uint64_t cur = (rem << 32) | t[j];
        t[j] = (uint32_t)(cur / d);
        rem = cur % d;
    }
    if (u256_gt(t, c.pow_limit)) {
#pragma unroll
        for (int j = 0; j < 8; j++) t[j] = c.pow_limit[j];
    }
    return compact_get(t);
}

// The status of header i of a round after its proof of work: hdr = the round's headers, hashes =
// its hash rows (8 words each), pow_ok = its proof-of-work bytes.
SHA_HD int header_context_lane(const uint8_t* hdr, const uint32_t* hashes, const uint8_t* pow_ok,
                               uint32_t i, const HeaderRoundCtx& c) {
    if (!pow_ok[i]) return BCC_HEADER_HIGH_HASH;
    if (i == 0 && c.genesis0) return BCC_HEADER_OK;
    const uint8_t* h = hdr + (size_t)HEADER_BYTES * i;
    const uint8_t* before = i ? h - HEADER_BYTES : h;  // read only when i > 0

    bool linked = true;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t want = i ? hashes[8 * (size_t)(i - 1) + j] : c.prev_hash[j];
        linked &= hdr_word(h, HW_PREV + j) == want;
    }
    if (!linked) return BCC_HEADER_PREV_MISMATCH;

    const uint32_t prev_bits = i ? hdr_word(before, HW_BITS) : c.prev_bits;
    const uint32_t prev_time = i ? hdr_word(before, HW_TIME) : c.times[0];
    const int64_t height = (int64_t)c.height0 + i;
    uint32_t want_bits = prev_bits;
    if (height % c.interval == 0) {
        const uint32_t first = i >= c.interval
                                   ? hdr_word(hdr + (size_t)HEADER_BYTES * (i - c.interval), HW_TIME)
                                   : c.period_first_time;
        want_bits = next_work_required(prev_bits, prev_time, first, c);
    }
    if (hdr_word(h, HW_BITS) != want_bits) return BCC_HEADER_BAD_DIFFBITS;

    // GetMedianTimePast: element m / 2 of the sorted up-to-11 times before this header, picked by
    // rank (ties by position) so that no array is indexed by a run-time value
    uint32_t t[MTP_SPAN], m = 0;
#pragma unroll
    for (uint32_t k = 0; k < MTP_SPAN; k++) {
        t[k] = 0;
        if (k < i) {
            t[k] = hdr_word(h - (size_t)HEADER_BYTES * (k + 1), HW_TIME);
            m = k + 1;
        } else if (k - i < c.n_times) {
            t[k] = c.times[k - i];
            m = k + 1;
        }
    }
    const uint32_t time = hdr_word(h, HW_TIME);
    uint32_t median = 0;
#pragma unroll
    for (uint32_t a = 0; a < MTP_SPAN; a++) {
        uint32_t rank = 0;
#pragma unroll
        for (uint32_t b = 0; b < MTP_SPAN; b++)
            rank += (b < m && (t[b] < t[a] || (t[b] == t[a] && b < a))) ? 1u : 0u;
        if (a < m && rank == m / 2) median = t[a];
    }
    if (m && time <= median) return BCC_HEADER_TIME_TOO_OLD;
    if (c.max_time != 0 && (int64_t)time > c.max_time) return BCC_HEADER_TIME_TOO_NEW;

    const int32_t version = (int32_t)hdr_word(h, HW_VERSION);
    if ((version < 2 && height >= c.bip34) || (version < 3 && height >= c.bip66) ||
        (version < 4 && height >= c.bip65))
        return BCC_HEADER_BAD_VERSION;
    return BCC_HEADER_OK;
}

// One round of bcc_headers_batch: n consecutive headers in the caller's memory, the context of the
// first, and where the hash rows (32 n bytes) and status words (n) go.
struct HeaderRound {
    const uint8_t* headers = nullptr;
    size_t n = 0;
    HeaderRoundCtx ctx{};
    uint8_t* hashes = nullptr;
    int* status = nullptr;
};
// One round of mi_pow_check_tuples.
struct PowRound {
    const uint8_t* hash32 = nullptr;
    const uint32_t* bits = nullptr;
    size_t n = 0;
    uint32_t pow_limit[8] = {};
    uint8_t* ok = nullptr;
};

// The device route, set by header_check.hip when the library loads; null in a build without the
// kernels (the CPU tests' engine), where a device round is the host evaluation.  The rounds
// return 0 or the HIP error; timing_ms: the calling thread's event times since reset (HEADER_MS_*;
// zero without BCC_HEADER_TIMING=1 in the environment).
enum { HEADER_MS_HASH = 0, HEADER_MS_CONTEXT, HEADER_MS_UPLOAD, HEADER_MS_DOWNLOAD, HEADER_MS_COUNT };
struct HeaderDeviceHook {
    int (*round)(int device, HeaderRound& r);
    int (*pow_round)(int device, PowRound& r);
    void (*timing_ms)(double* ms, int reset);  // ms may be null
};
extern const HeaderDeviceHook* g_header_device_hook;

namespace host {
// The same rounds on the host: the lane code above over the calling thread's team.
void header_round_host(HeaderRound& r);
void pow_round_host(PowRound& r);
}  // namespace host

}  // namespace bcc
