// Header chains in batch: bcc_headers_batch and mi_pow_check_tuples (include/bcc_amd.h).
//
// Host half: the argument rules, the round loop, what a round's first headers need from before it
// (header_context_at, the one place that says so), the chain-work sum (GetBlockProof,
// chain.cpp:122-135) and the host evaluation of a round.  A round runs on the device through
// g_header_device_hook (header_check.hip), or here on the host over the same records
// (header_round_host: the kernels' lane code on the calling thread's team): rounds of at most the
// small-round threshold, and rounds the device could not deliver (the Taproot side's failure
// rules, taproot_host.h).
#include <algorithm>
#include <atomic>
#include <cstring>
#include <functional>
#include <vector>

#include "../header_check.h"
#include "bcc_amd.h"
#include "devices.h"
#include "hashes.h"
#include "host_verify.h"
#include "taproot_host.h"
#include "tuples.h"

namespace bcc {

const HeaderDeviceHook* g_header_device_hook = nullptr;

namespace host {
namespace {

// Headers per device round when bcc_set_header_round is 0: a 20 MiB upload.
constexpr size_t HEADER_ROUND = (size_t)1 << 18;
// Headers per device share of a call with device = -1.
constexpr size_t DEVICE_SHARE_HEADERS = 256;
// The small-round thresholds.  Headers: measured, the host route won up to 128
// headers and the device from 192.  Rows of mi_pow_check_tuples: not measured, the block entries'
// provisional figure.
#ifndef BCC_HEADER_SMALL_ROUND
#define BCC_HEADER_SMALL_ROUND 128
#endif
#ifndef BCC_POW_SMALL_ROUND
#define BCC_POW_SMALL_ROUND 2048
#endif

std::atomic<size_t> g_header_round{0};
thread_local bcc_header_stats t_header_stats{};

size_t header_round_size() {
    const size_t r = g_header_round.load(std::memory_order_relaxed);
    return r ? r : HEADER_ROUND;
}
// 0 with bcc_set_host_small_round(0); else the entry's own threshold, or the caller's larger one
size_t small_round(size_t own) {
    const size_t s = host_small_round();
    return s ? std::max(s, own) : 0;
}

void store_stats(size_t headers, const TaprootCounters& c) {
    bcc_header_stats s{};
    s.headers = headers;
    s.host_rounds = c.host_rounds.load();
    s.device_rounds = c.rounds.load() - s.host_rounds;
    s.device_retries = c.device_retries.load();
    t_header_stats = s;
}

uint32_t le32(const uint8_t* p) { return hdr_word(p, 0); }

// What the lanes of a round that starts at header g read from before it.  Everything comes from
// the header bytes themselves or from the anchor, never from another round's results, so a round
// may be cut anywhere and the ranges of a device list need nothing from each other.
void header_context_at(HeaderRoundCtx& c, const uint8_t* headers, size_t g,
                       const bcc_header_anchor* anchor) {
    const int64_t height_of_0 = anchor ? (int64_t)anchor->height + 1 : 0;
    c.height0 = (int32_t)(height_of_0 + (int64_t)g);
    c.genesis0 = !anchor && g == 0;
    c.prev_bits = 0;
    memset(c.prev_hash, 0, sizeof c.prev_hash);
    if (g) {
        const uint8_t* before = headers + HEADER_BYTES * (g - 1);
        uint8_t hash[32];
        sha256d(before, HEADER_BYTES, hash);
        memcpy(c.prev_hash, hash, 32);
        c.prev_bits = hdr_word(before, HW_BITS);
    } else if (anchor) {
        memcpy(c.prev_hash, anchor->hash, 32);
        c.prev_bits = anchor->bits;
    }
    c.n_times = 0;
    for (size_t k = 0; k < MTP_SPAN; k++) {
        c.times[k] = 0;
        if (k < g) c.times[k] = hdr_word(headers + HEADER_BYTES * (g - 1 - k), HW_TIME);
        else if (anchor && k - g < anchor->n_times) c.times[k] = anchor->times[k - g];
        else continue;
        c.n_times = (uint32_t)k + 1;
    }
    // the first boundary at or above the round's first height, and the block `interval` below it
    const int64_t boundary = (c.height0 + (int64_t)c.interval - 1) / c.interval * c.interval;
    const int64_t first = boundary - c.interval - height_of_0;  // as an index into headers
    c.period_first_time = 0;
    if (first >= 0 && (size_t)first < g)
        c.period_first_time = hdr_word(headers + HEADER_BYTES * (size_t)first, HW_TIME);
    else if (first < 0 && anchor)
        c.period_first_time = anchor->period_first_time;
}

// ---- GetBlockProof and the 256-bit sum ----------------------------------------------------------

using U256 = uint32_t[8];

bool u256_ge(const U256& a, const U256& b) { return !u256_gt(b, a); }
void u256_sub(U256& a, const U256& b) {
    uint64_t borrow = 0;
    for (int j = 0; j < 8; j++) {
        const uint64_t d = (uint64_t)a[j] - b[j] - borrow;
        a[j] = (uint32_t)d;
        borrow = (d >> 32) & 1;
    }
}
void u256_add(U256& a, const U256& b) {
    uint64_t carry = 0;
    for (int j = 0; j < 8; j++) {
        const uint64_t s = (uint64_t)a[j] + b[j] + carry;
        a[j] = (uint32_t)s;
        carry = s >> 32;
    }
}
// ~t / (t + 1) + 1; zero where GetBlockProof returns zero
void block_proof(uint32_t bits, U256& out) {
    U256 t, den, num, rem = {};
    memset(out, 0, sizeof(U256));
    if (compact_expand(bits, t) || u256_zero(t)) return;
    const U256 one = {1};
    memcpy(den, t, sizeof den);
    u256_add(den, one);  // t < 2^256 - 1 here: a valid target has at most 23 + 8 * 29 bits
    for (int j = 0; j < 8; j++) num[j] = ~t[j];
    for (int bit = 255; bit >= 0; bit--) {  // schoolbook: rem = rem * 2 + the next bit of num
        const uint32_t top = rem[7] >> 31;
        for (int j = 7; j > 0; j--) rem[j] = (rem[j] << 1) | (rem[j - 1] >> 31);
        rem[0] = (rem[0] << 1) | ((num[bit / 32] >> (bit % 32)) & 1u);
        if (top || u256_ge(rem, den)) {
            u256_sub(rem, den);
            out[bit / 32] |= 1u << (bit % 32);
        }
    }
    u256_add(out, one);
}

// ---- the rounds -----------------------------------------------------------------------------------

struct RangeState {
    int device;
    DeviceRange fail;
    TaprootCounters& c;
};

// A round under the failure rules: on the host when it is small, else on the device with one
// retry and the policy.
int run_round(const char* who, size_t rows, size_t small, RangeState& rs,
              const std::function<int()>& on_device, const std::function<void()>& on_host) {
    if (rows <= small_round(small)) {
        on_host();
        rs.c.round(rows, 0, true);
        return 0;
    }
    return resilient_taproot_round(who, rs.device, rows, 0, rs.fail, rs.c, on_device, on_host);
}

// Headers [lo, hi) on one device, in rounds.
int headers_range(const uint8_t* headers, size_t lo, size_t hi, const HeaderRoundCtx& params,
                  const bcc_header_anchor* anchor, uint8_t* hashes, int* status, RangeState& rs) {
    const size_t per = header_round_size();
    for (size_t g = lo; g < hi; g += std::min(per, hi - g)) {
        HeaderRound r;
        r.headers = headers + HEADER_BYTES * g;
        r.n = std::min(per, hi - g);
        r.ctx = params;
        header_context_at(r.ctx, headers, g, anchor);
        r.hashes = hashes + 32 * g;
        r.status = status + g;
        const HeaderDeviceHook* hook = g_header_device_hook;
        const int e = run_round("headers_batch", r.n, BCC_HEADER_SMALL_ROUND, rs, [&] {
            if (hook) return hook->round(rs.device, r);
            header_round_host(r);  // a build without the kernels
            return 0;
        }, [&] { header_round_host(r); });
        if (e) return e;
    }
    return 0;
}

void limbs_of(const unsigned char* bytes32, uint32_t (&out)[8]) {
    for (int j = 0; j < 8; j++) out[j] = le32(bytes32 + 4 * j);
}

}  // namespace

void header_round_host(HeaderRound& r) {
    std::vector<uint8_t> pow_ok(r.n);
    pfor(r.n, 256, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) {
            uint32_t h[HEADER_WORDS], d[8];
            for (uint32_t k = 0; k < HEADER_WORDS; k++) h[k] = hdr_word(r.headers + HEADER_BYTES * i, k);
            header_hash_lane(h, d);
            memcpy(r.hashes + 32 * i, d, 32);
            pow_ok[i] = pow_check(d, h[HW_BITS], r.ctx.pow_limit) ? 1 : 0;
        }
    });
    // the hash rows as the context lanes read them (the caller's buffer may sit at any address)
    std::vector<uint32_t> rows(8 * r.n);
    memcpy(rows.data(), r.hashes, 32 * r.n);
    pfor(r.n, 1024, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++)
            r.status[i] = header_context_lane(r.headers, rows.data(), pow_ok.data(), (uint32_t)i, r.ctx);
    });
}

void pow_round_host(PowRound& r) {
    pfor(r.n, 1024, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) {
            uint32_t d[8];
            memcpy(d, r.hash32 + 32 * i, 32);
            uint32_t bits;
            memcpy(&bits, (const uint8_t*)r.bits + 4 * i, 4);
            r.ok[i] = pow_check(d, bits, r.pow_limit) ? 1 : 0;
        }
    });
}

}  // namespace host
}  // namespace bcc

using namespace bcc;
using namespace bcc::host;

extern "C" {

long bcc_headers_batch(const unsigned char* headers80, size_t n, const bcc_header_params* params,
                       const bcc_header_anchor* anchor, int64_t max_time, unsigned char* hash_out,
                       int* status_out, unsigned char* chain_work_out, int device) {
    if (chain_work_out) memset(chain_work_out, 0, 32);
    if (n == 0) return 0;
    if (!headers80 || !params || !status_out) return -1;
    const bcc_header_params& P = *params;
    if (P.pow_allow_min_difficulty || P.pow_target_spacing <= 0 || P.pow_target_timespan <= 0 ||
        P.pow_target_timespan >= ((int64_t)1 << 30) || P.pow_target_timespan / P.pow_target_spacing < 1)
        return -1;
    if (anchor && (anchor->height < 0 || anchor->n_times < 1 || anchor->n_times > MTP_SPAN)) return -1;
    if ((anchor ? (uint64_t)anchor->height + 1 : 0) + (uint64_t)n > (uint64_t)INT32_MAX + 1) return -1;

    HeaderRoundCtx base{};
    limbs_of(P.pow_limit, base.pow_limit);
    base.timespan = P.pow_target_timespan;
    base.max_time = max_time;
    base.interval = (uint32_t)(P.pow_target_timespan / P.pow_target_spacing);
    base.no_retarget = P.pow_no_retargeting ? 1 : 0;
    base.bip34 = P.bip34_height;
    base.bip66 = P.bip66_height;
    base.bip65 = P.bip65_height;

    std::vector<uint8_t> own_hashes;
    if (!hash_out) {
        own_hashes.resize(32 * n);
        hash_out = own_hashes.data();
    }
    if (g_header_device_hook) g_header_device_hook->timing_ms(nullptr, 1);
    TaprootCounters c;
    int rc;
    {
        ActiveCaller active;
        const std::vector<int> devs = device < 0 ? device_list() : std::vector<int>{device};
        const size_t D = std::max<size_t>(
            1, std::min(devs.size(), (n + DEVICE_SHARE_HEADERS - 1) / DEVICE_SHARE_HEADERS));
        std::vector<std::function<int()>> jobs;
        std::vector<int> used;
        for (size_t d = 0; d < D; d++) {
            const size_t lo = n * d / D, hi = n * (d + 1) / D;
            const int dev = devs[d];
            used.push_back(dev);
            jobs.push_back([=, &c, &base] {
                RangeState rs{dev, {}, c};
                return headers_range(headers80, lo, hi, base, anchor, hash_out, status_out, rs);
            });
        }
        rc = run_on_devices(used, jobs);
    }
    store_stats(n, c);
    if (rc) return -1;

    size_t first_bad = 0;
    while (first_bad < n && status_out[first_bad] == BCC_HEADER_OK) first_bad++;
    if (chain_work_out) {  // one division per run of equal nBits
        U256 sum = {}, proof = {};
        uint32_t run_bits = 0;
        for (size_t i = 0; i < first_bad; i++) {
            const uint32_t bits = hdr_word(headers80 + HEADER_BYTES * i, HW_BITS);
            if (i == 0 || bits != run_bits) block_proof(run_bits = bits, proof);
            u256_add(sum, proof);
        }
        memcpy(chain_work_out, sum, 32);
    }
    return (long)first_bad;
}

int mi_pow_check_tuples(const unsigned char* hash32, const uint32_t* bits, size_t n,
                        const unsigned char* pow_limit, unsigned char* ok_out, int device) {
    if (n == 0) return 0;
    if (!hash32 || !bits || !pow_limit || !ok_out) return -1;
    ActiveCaller active;
    TaprootCounters c;
    RangeState rs{device < 0 ? device_list()[0] : device, {}, c};
    const size_t per = header_round_size();
    int rc = 0;
    for (size_t g = 0; g < n && !rc; g += per) {
        PowRound r;
        r.hash32 = hash32 + 32 * g;
        r.bits = (const uint32_t*)((const uint8_t*)bits + 4 * g);
        r.n = std::min(per, n - g);
        limbs_of(pow_limit, r.pow_limit);
        r.ok = ok_out + g;
        const HeaderDeviceHook* hook = g_header_device_hook;
        rc = run_round("pow_check_tuples", r.n, BCC_POW_SMALL_ROUND, rs, [&] {
            if (hook) return hook->pow_round(rs.device, r);
            pow_round_host(r);
            return 0;
        }, [&] { pow_round_host(r); });
    }
    store_stats(n, c);
    return rc;
}

void bcc_last_header_stats(bcc_header_stats* out) {
    if (out) *out = t_header_stats;
}

int bcc_set_header_round(size_t headers) {
    g_header_round.store(headers, std::memory_order_relaxed);
    return 0;
}

void bcc_header_last_timing_ms(double* ms4) {
    if (!ms4) return;
    for (int k = 0; k < HEADER_MS_COUNT; k++) ms4[k] = 0;
    if (g_header_device_hook) g_header_device_hook->timing_ms(ms4, 0);
}

}  // extern "C"
