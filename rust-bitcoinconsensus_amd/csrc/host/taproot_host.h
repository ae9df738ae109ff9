// The Taproot side on the host CPU (taproot_host.cpp): a Taproot device round evaluated by host
// code (the kernels' BIP340 lane over the host comb, host SHA-256 over the very job records the
// device reads), the failure rules every Taproot entry point applies to a device round (injected
// fault, one retry, failure policy: resilient_round's, engine.h), and the statistics of the
// calling thread's last Taproot-side call (bcc_last_taproot_stats).
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <functional>

#include "../pipeline.h"
#include "bcc_amd.h"

namespace bcc {
namespace host {

// gpu_taproot_verify_parts on the host: one verdict byte per row of the concatenated parts and,
// with msg32_out, each row's 32-byte sighash.  BIP340 runs on up to `threads` team threads.
void host_taproot_parts(const TaprootJobs* const* parts, size_t P, uint8_t* verdict,
                        uint8_t* msg32_out, unsigned threads);

// mi_schnorr_verify_tuples' rows on the host (secp256k1_schnorrsig_verify per row).
void host_schnorr_rows(const uint8_t* sig64, const uint8_t* msg32, const uint8_t* xonly32,
                       uint8_t* verdict, size_t n, unsigned threads);

// The counters of one Taproot-side call, summed over its device ranges (which may run on the
// per-GPU worker threads); taproot_stats_store makes them the calling thread's last call.
struct TaprootCounters {
    std::atomic<size_t> checks{0}, commits{0}, rounds{0}, host_rounds{0}, host_checks{0},
        device_retries{0};
    // one round of `rows` signature rows and `commits` commitment lanes; on_host: the host ran it
    void round(size_t rows, size_t commit_lanes, bool on_host) {
        checks += rows;
        commits += commit_lanes;
        rounds++;
        if (on_host) {
            host_rounds++;
            host_checks += rows + commit_lanes;
        }
    }
};
void taproot_stats_store(size_t items, const TaprootCounters& c);
// (bcc_verify_inputs_batch runs its v1 side on another thread and hands that thread's last call
// to its caller)
void taproot_stats_set(const bcc_taproot_stats& s);

// The failure state of one device range of a call: after a device error that no retry can cure
// the context is unusable, and the range's remaining rounds go straight to the policy.  An
// injected fault (bcc_debug_fail_device_rounds_code) never reached the GPU and leaves the context
// as it was, so it fails its own round only.
struct DeviceRange {
    int sticky = 0;
    bool injected = false;  // the error round_blocked last returned was an injected one
};

// A device round that failed at its begin or its end, as the failure rules need it.
struct FailedRound {
    std::function<void()> rebuild;        // its parts again from its items (null: they are intact)
    std::function<size_t()> checks;       // signature rows + commitments (after the rebuild)
    std::function<int()> run;             // begin and end, synchronously: 0 or the HIP error
    std::function<void()> host;           // the same round evaluated on the host
    std::function<void(bool on_host)> done;  // counts the round and applies its verdicts
    std::function<void()> lost;           // (optional) no verdict: BCC_DEVICE_FAILURE_ERROR
};
// The rules, given the round's error e (nonzero): a transient e is worth one re-run (counted in
// c.device_retries, logged); otherwise, or if the re-run fails, the policy decides: the host
// evaluation (logged, bcc_host_fallback_rounds), or e is returned.  A non-retryable e from the
// device makes the range sticky.  Returns 0 or the error.
int recover_round(const char* who, int dev, int e, DeviceRange& range, TaprootCounters& c,
                  const FailedRound& r);

// A pending injected fault or the range's sticky error, else 0: asked before a round is begun.
int round_blocked(DeviceRange& range);

// One synchronous round under those rules: device() runs it on the GPU and returns 0 or the HIP
// error; host() computes the same on the CPU.  Counts the round (`rows` signature rows, `commits`
// commitment lanes).  Returns 0, or the error under BCC_DEVICE_FAILURE_ERROR.
int resilient_taproot_round(const char* who, int dev, size_t rows, size_t commits,
                            DeviceRange& range, TaprootCounters& c,
                            const std::function<int()>& device, const std::function<void()>& host);

// bcc_taproot_spend_batch with one more output: unfinished[i] = 1 (optional, n bytes) for every
// item a failed call left without a verdict (BCC_DEVICE_FAILURE_ERROR); the rest are final.
int taproot_spend_run(const bcc_taproot_spend* items, size_t n, int* ret_out, int* serror_out,
                      int device, uint8_t* unfinished);

}  // namespace host
}  // namespace bcc
