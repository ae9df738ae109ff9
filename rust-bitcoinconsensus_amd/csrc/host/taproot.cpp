// BIP341 / BIP342 signature checks in batch: bcc_taproot_verify_batch (include/bcc_amd.h).
//
// Host half of GenericTransactionSignatureChecker::CheckSchnorrSignature
// (interpreter.cpp:1678-1704) and SignatureHashSchnorr (:1491-1574): the size / hash_type
// rules, the SigMsg serialization with 32-byte slots for every hash, and the single-SHA-256 aux
// messages those slots take (PrecomputedTransactionData::Init's sha_prevouts / sha_amounts /
// sha_scriptpubkeys / sha_sequences / sha_outputs, :1366-1417 and :1455-1471, once per adjacent
// run of items with the same tx; a check's sha_annex, :1889-1893, and sha_single_output,
// :1556-1561).  Every SHA-256 compression and the BIP340 verification run on the GPU
// (taproot_round.hip gpu_taproot_verify over sighash.hip's kernels: aux hashes, digest patching, TapSighash from the tag
// midstate, then the Schnorr kernels); a round of at most bcc_set_host_small_round() checks, and a
// round the device could not deliver, is evaluated by the host instead (taproot_host.h).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>

#include "bcc_amd.h"
#include "devices.h"
#include "engine.h"
#include "hashes.h"
#include "host_verify.h"
#include "taproot_host.h"
#include "taproot_jobs.h"
#include "team.h"
#include "tuples.h"
#include "tx.h"

namespace bcc {
namespace host {
namespace {

constexpr int SCRIPT_ERR_UNKNOWN_ERROR = 1;

// One part of a round: the jobs of a contiguous item range (built by one host thread).
struct alignas(64) Part {  // one per worker, appended per check: no cache line shared with the next
    TaprootJobs jobs;
    std::vector<uint32_t> item_of_row;  // row -> item index (absolute)
};

// job parts of the calling thread (run_range; released by bcc_release_thread_state)
thread_local std::vector<Part> tl_parts;

// A launched round of the pipelined run_range: its rows' items and the verdict / sighash buffers.
struct RoundOut {
    std::vector<uint32_t> item_of_row;
    std::vector<uint8_t> verdict, msg;
};
thread_local RoundOut tl_round_out[TAPROOT_SLOTS];

// Items [lo, hi): resolve on the host what needs no hashing, build the SigMsg jobs for the rest.
void build_part(const bcc_taproot_check* items, size_t lo, size_t hi, int* ret, int* serr,
                Part& P) {
    TaprootJobs& J = P.jobs;
    J.clear();
    P.item_of_row.clear();
    const size_t cnt = hi - lo;  // capacity for the common shape (a key path spend of its own tx)
    J.dev.txraw.reserve(cnt * 200);
    J.dev.ttx.reserve(cnt);
    J.dev.jobs.reserve(cnt);
    J.sig64.reserve(cnt * 64);
    J.pk32.reserve(cnt * 32);
    P.item_of_row.reserve(cnt);
    TxState s;
    std::vector<uint8_t> scratch;
    for (size_t i = lo; i < hi; i++) {
        const bcc_taproot_check& it = items[i];
        ret[i] = 0;
        serr[i] = 0;
        if (!load_tx(s, it.tx, it.tx_len, it.spent_outputs, it.spent_outputs_len) ||
            it.n_in >= s.t.vin.size() || !it.pubkey32 || (it.sig_len && !it.sig) ||
            (it.sigversion != BCC_SIGVERSION_TAPROOT && it.sigversion != BCC_SIGVERSION_TAPSCRIPT) ||
            (it.sigversion == BCC_SIGVERSION_TAPSCRIPT && !it.tapleaf_hash32)) {
            ret[i] = -1;
            serr[i] = SCRIPT_ERR_UNKNOWN_ERROR;
            continue;
        }
        if (int e = taproot_add_check(s, J, it.n_in, it.sig, it.sig_len, it.pubkey32,
                                      it.sigversion == BCC_SIGVERSION_TAPSCRIPT, it.annex,
                                      it.annex_len, it.tapleaf_hash32, it.codeseparator_pos, scratch)) {
            serr[i] = e;
            continue;
        }
        P.item_of_row.push_back((uint32_t)i);
    }
}

// Builds the parts of items [lo, hi) in parallel on the calling thread's team (tl_parts).
// Returns the number of parts, or 0 when the round's message blobs would not fit the kernels'
// 32-bit offsets (the caller splits it).
size_t build_round(const bcc_taproot_check* items, size_t lo, size_t hi, int* ret, int* serr) {
    // parts: contiguous item ranges, cut only between runs of the same tx
    const unsigned T = pool_threads(hi - lo, 2048);
    std::vector<size_t> cut{lo};
    for (unsigned t = 1; t < T; t++) {
        size_t c = std::max(cut.back(), lo + (hi - lo) * t / T);
        while (c > cut.back() && c < hi && items[c].tx == items[c - 1].tx) c++;
        if (c > cut.back() && c < hi) cut.push_back(c);
    }
    cut.push_back(hi);
    // the parts live with the calling thread and keep their capacity across calls: a 1M-check
    // round fills ~650 MB of job blobs, which fresh vectors would page-fault in every call
    std::vector<Part>& parts = tl_parts;
    if (parts.size() < cut.size() - 1) parts.resize(cut.size() - 1);
    run_team((unsigned)(cut.size() - 1), [&](unsigned p) {
        build_part(items, cut[p], cut[p + 1], ret, serr, parts[p]);
    });
    const size_t NP = cut.size() - 1;
    size_t aux_b = 0, msg_b = 0;
    for (size_t p = 0; p < NP; p++) {
        aux_b += parts[p].jobs.aux.size() + parts[p].jobs.dev.ext.size();
        msg_b += parts[p].jobs.msg.size() + parts[p].jobs.dev.txraw.size();
    }
    if (aux_b >= ((size_t)1 << 32) || msg_b >= ((size_t)1 << 32)) return 0;
    return NP;
}

// The round built in tl_parts (NP parts): its job parts, and its row -> item map into out (with the
// verdict / sighash buffers sized for it).  Returns the number of rows.
size_t collect_round(size_t NP, RoundOut& out, std::vector<const TaprootJobs*>& pj,
                     bool sighashes) {
    pj.clear();
    out.item_of_row.clear();
    for (size_t p = 0; p < NP; p++) {
        const Part& q = tl_parts[p];
        pj.push_back(&q.jobs);
        out.item_of_row.insert(out.item_of_row.end(), q.item_of_row.begin(), q.item_of_row.end());
    }
    const size_t n = out.item_of_row.size();
    out.verdict.resize(n);  // (every byte is written by the round's evaluation, device or host)
    out.msg.resize(sighashes ? 32 * n : 0);
    return n;
}

// A finished round's verdicts (and sighashes) onto its items.
void scatter_round(RoundOut& out, int* ret, int* serr, unsigned char* sighash_out) {
    const size_t n = out.item_of_row.size();
    for (size_t r = 0; r < n; r++) {
        const uint32_t i = out.item_of_row[r];
        ret[i] = out.verdict[r] ? 1 : 0;
        serr[i] = out.verdict[r] ? 0 : BCC_SCRIPT_ERR_SCHNORR_SIG;
        if (sighash_out) memcpy(sighash_out + 32 * (size_t)i, &out.msg[32 * r], 32);
    }
    out.item_of_row.clear();
}

// What one device range of a call carries from round to round.
struct RangeState {
    int device;
    DeviceRange fail;
    TaprootCounters& c;
};
constexpr const char* WHO = "taproot_verify_batch";

// Items [lo, hi) on `device` as one GPU round: host parts in parallel, verdicts scattered back.
// A round whose message blobs would not fit the kernels' 32-bit offsets is split in two.  A round
// of at most host_small_round() rows runs on the host; a round the device cannot deliver is
// retried once and then goes to the failure policy.
int run_range(const bcc_taproot_check* items, size_t lo, size_t hi, int* ret, int* serr,
              unsigned char* sighash_out, RangeState& rs) {
    if (lo >= hi) return 0;
    if (sighash_out)
        for (size_t i = lo; i < hi; i++) memset(sighash_out + 32 * i, 0, 32);
    const size_t NP = build_round(items, lo, hi, ret, serr);
    if (NP == 0 && hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (int e = run_range(items, lo, mid, ret, serr, sighash_out, rs)) return e;
        return run_range(items, mid, hi, ret, serr, sighash_out, rs);
    }
    RoundOut& out = tl_round_out[0];
    std::vector<const TaprootJobs*> pj;
    const size_t rows = collect_round(NP, out, pj, sighash_out != nullptr);
    if (rows == 0) return 0;
    uint8_t* msg = sighash_out ? out.msg.data() : nullptr;
    auto on_host = [&] {
        host_taproot_parts(pj.data(), pj.size(), out.verdict.data(), msg, host_threads());
    };
    if (rows <= host_small_round()) {  // latency: no device state is touched
        on_host();
        rs.c.round(rows, 0, true);
    } else if (int e = resilient_taproot_round(WHO, rs.device, rows, 0, rs.fail, rs.c, [&] {
                   return gpu_taproot_verify_parts(rs.device, pj.data(), pj.size(),
                                                   out.verdict.data(), msg);
               }, on_host)) {
        return e;
    }
    scatter_round(out, ret, serr, sighash_out);
    return 0;
}

// Rounds of about PIPE_ROUND checks, pipelined (a batch of at least two): round k's host parts
// are built while rounds k - 1 and k - 2 are on the GPU (TAPROOT_SLOTS = 3 contexts), and round
// k's upload runs beside their kernels.  Round 4 had two slots (16-19 ms per 1M checks in 131,072
// rounds, profiles/r04/c5t): round k + 1 was built only after round k - 1 finished, and round k - 1's
// verdict copy queued behind round k's upload in the one copy queue (profiles/r05/c5t timelines).
// Round 5: verdicts written to pinned memory by a kernel behind the round (gpu_taproot_begin), three
// slots, 65,536-check rounds (two overlap on the GPU): 13.3-13.9 ms per 1M (131,072: 13.5-15.7;
// 81,920: 14.9-15.9; 49,152: 15.0-17.6; profiles/r05/c5t/rounds.txt).
#ifndef BCC_TAPROOT_PIPE_ROUND
#define BCC_TAPROOT_PIPE_ROUND 65536
#endif
static const size_t PIPE_ROUND = [] {  // BCC_TAPROOT_ROUND overrides (experiments)
    const char* e = getenv("BCC_TAPROOT_ROUND");
    return e && atoll(e) > 0 ? (size_t)atoll(e) : (size_t)BCC_TAPROOT_PIPE_ROUND;
}();
static const bool g_tap_trace = getenv("BCC_TAPROOT_TRACE") != nullptr;

int run_pipelined(const bcc_taproot_check* items, size_t lo, size_t hi, int* ret, int* serr,
                  unsigned char* sighash_out, RangeState& rs) {
    if (hi - lo < 2 * PIPE_ROUND) return run_range(items, lo, hi, ret, serr, sighash_out, rs);
    const int device = rs.device;
    if (sighash_out)
        for (size_t i = lo; i < hi; i++) memset(sighash_out + 32 * i, 0, 32);
    std::vector<size_t> cut{lo};
    while (cut.back() < hi) {
        size_t c = std::min(hi, cut.back() + PIPE_ROUND);
        while (c < hi && items[c].tx == items[c - 1].tx) c++;
        cut.push_back(c);
    }
    // rounds in flight: launched, not yet finished (at most TAPROOT_SLOTS - 1 while the host builds
    // the next: round k is launched before round k - 2 is finished)
    struct Flight {
        int slot;
        size_t lo, hi;  // its item range: a failed round is rebuilt from it
    };
    std::vector<Flight> inflight;
    int err = 0;
    std::vector<const TaprootJobs*> pj;
    // Round f failed with e at its begin (the parts in tl_parts are still its own) or at its end
    // (by then tl_parts hold a later round's build, so the round is rebuilt from its items: the
    // build is deterministic).  recover_round re-runs it once on the slot's fresh context if e is
    // transient, and else leaves it to the policy.
    auto recover = [&](const Flight& f, int e, bool parts_intact) -> int {
        RoundOut& out = tl_round_out[f.slot];
        FailedRound r;
        if (!parts_intact)
            r.rebuild = [&] {
                collect_round(build_round(items, f.lo, f.hi, ret, serr), out, pj, sighash_out != nullptr);
            };
        r.checks = [&] { return out.item_of_row.size(); };
        r.run = [&] {
            if (int e2 = gpu_taproot_begin(device, f.slot, pj.data(), pj.size())) return e2;
            return gpu_taproot_end(device, f.slot, out.verdict.data(),
                                   sighash_out ? out.msg.data() : nullptr);
        };
        r.host = [&] {
            host_taproot_parts(pj.data(), pj.size(), out.verdict.data(),
                               sighash_out ? out.msg.data() : nullptr, host_threads());
        };
        r.done = [&](bool on_host) {
            rs.c.round(out.item_of_row.size(), 0, on_host);
            scatter_round(out, ret, serr, sighash_out);
        };
        return recover_round(WHO, device, e, rs.fail, rs.c, r);
    };
    // Waits for a launched round and writes its verdicts to the items.
    auto finish = [&](const Flight& f) -> int {
        RoundOut& out = tl_round_out[f.slot];
        const size_t rows = out.item_of_row.size();
        if (rows == 0) return 0;
        if (int e = gpu_taproot_end(device, f.slot, out.verdict.data(),
                                    sighash_out ? out.msg.data() : nullptr))
            return recover(f, e, false);
        rs.c.round(rows, 0, false);
        scatter_round(out, ret, serr, sighash_out);
        return 0;
    };
    using clk = std::chrono::steady_clock;
    auto ms = [](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
    double t_build = 0, t_launch = 0, t_finish = 0;
    const auto c0 = clk::now();
    // slots rotate by LAUNCHED rounds: at most TAPROOT_SLOTS - 1 are in flight after a launch, so
    // the next launch's slot is never one of them (a round that launches nothing -- no rows, a
    // small round, a round the failure rules finished on the spot -- must not advance the rotation)
    size_t launched = 0;
    for (size_t k = 0; k + 1 < cut.size() && !err; k++) {
        const int slot = (int)(launched % TAPROOT_SLOTS);
        auto q = clk::now();
        auto ns = [](clk::time_point t) { return (long long)std::chrono::duration_cast<std::chrono::nanoseconds>(t.time_since_epoch()).count(); };
        if (g_tap_trace) fprintf(stderr, "[bcc] tap k=%zu build_start %lld\n", k, ns(q));
        const size_t NP = build_round(items, cut[k], cut[k + 1], ret, serr);
        t_build += ms(q);
        if (g_tap_trace) fprintf(stderr, "[bcc] tap k=%zu build_end %lld\n", k, ns(clk::now()));
        if (NP == 0) {  // too large for one launch: this round alone, unpipelined
            for (const Flight& f : inflight)
                if (int e = finish(f)) err = err ? err : e;
            inflight.clear();
            if (!err) err = run_range(items, cut[k], cut[k + 1], ret, serr, sighash_out, rs);
            continue;
        }
        q = clk::now();
        const Flight f{slot, cut[k], cut[k + 1]};
        RoundOut& out = tl_round_out[slot];
        const size_t rows = collect_round(NP, out, pj, sighash_out != nullptr);
        if (rows != 0 && rows <= host_small_round()) {  // a round in which few items reach BIP340
            host_taproot_parts(pj.data(), pj.size(), out.verdict.data(),
                               sighash_out ? out.msg.data() : nullptr, host_threads());
            rs.c.round(rows, 0, true);
            scatter_round(out, ret, serr, sighash_out);
        } else if (rows != 0) {
            // an injected fault, or an earlier error that left the context unusable, comes before
            // the launch: such a round never reaches the GPU
            int e = round_blocked(rs.fail);
            if (!e) e = gpu_taproot_begin(device, slot, pj.data(), pj.size());
            if (e) {
                err = recover(f, e, true);
            } else {
                inflight.push_back(f);
                launched++;
            }
        }
        t_launch += ms(q);
        if (g_tap_trace) fprintf(stderr, "[bcc] tap k=%zu launch_end %lld\n", k, ns(clk::now()));
        q = clk::now();
        while ((int)inflight.size() > TAPROOT_SLOTS - 1 || (err && !inflight.empty())) {
            const Flight p = inflight.front();
            inflight.erase(inflight.begin());
            const int e = finish(p);
            if (!err) err = e;
        }
        t_finish += ms(q);
        if (g_tap_trace) fprintf(stderr, "[bcc] tap k=%zu finish_prev_end %lld\n", k, ns(clk::now()));
    }
    auto q = clk::now();
    for (const Flight& f : inflight) {  // in launch order; every launched round is ended, even after an error
        const int e = finish(f);
        if (!err) err = e;
    }
    t_finish += ms(q);
    if (g_tap_trace)
        fprintf(stderr, "[bcc] taproot rounds: %zu checks, %zu rounds, %.2f ms: build %.2f launch(stage+issue) %.2f finish(wait) %.2f ms\n",
                hi - lo, cut.size() - 1, ms(c0), t_build, t_launch, t_finish);
    return err;
}

}  // namespace

void taproot_release_thread_state() {
    std::vector<Part>().swap(tl_parts);
    for (auto& o : tl_round_out) o = RoundOut();
}

}  // namespace host
}  // namespace bcc

extern "C" int bcc_taproot_verify_batch(const bcc_taproot_check* items, size_t n, int* ret_out,
                                        int* serror_out, unsigned char* sighash_out, int device) {
    if (n == 0) return 0;
    if (!items || !ret_out || !serror_out) return -1;
    bcc::host::ActiveCaller active;
    std::vector<int> devs = device < 0 ? bcc::host::device_list() : std::vector<int>{device};
    const size_t D = std::max<size_t>(1, std::min<size_t>(devs.size(), (n + 4095) / 4096));
    // contiguous item ranges per device, cut only between runs of the same tx
    std::vector<size_t> cut{0};
    for (size_t d = 1; d < D; d++) {
        size_t c = std::max(cut.back(), n * d / D);
        while (c > cut.back() && c < n && items[c].tx == items[c - 1].tx) c++;
        if (c > cut.back() && c < n) cut.push_back(c);
    }
    cut.push_back(n);
    // rounds of at most 4M items per device bound the staged blobs and the kernel scratch
    constexpr size_t ROUND = (size_t)4 << 20;
    bcc::host::TaprootCounters counters;
    std::vector<std::function<int()>> jobs;
    for (size_t d = 0; d + 1 < cut.size(); d++) {
        const size_t lo = cut[d], hi = cut[d + 1];
        const int dev = devs[d];
        jobs.push_back([=, &counters] {
            bcc::host::RangeState rs{dev, {}, counters};
            for (size_t r = lo; r < hi; r += ROUND)
                if (int e = bcc::host::run_pipelined(items, r, std::min(hi, r + ROUND), ret_out,
                                                     serror_out, sighash_out, rs))
                    return e;
            return 0;
        });
    }
    devs.resize(jobs.size());
    const int rc = bcc::host::run_on_devices(devs, jobs);
    bcc::host::taproot_stats_store(n, counters);
    return rc ? -1 : 0;
}
