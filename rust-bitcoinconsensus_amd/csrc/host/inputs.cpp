// Any input against the outputs its transaction spends: bcc_verify_inputs_batch (include/bcc_amd.h).
//
// The engine has two batched verifiers with two item shapes: bitcoinconsensus_verify_batch
// (engine.cpp: every kind of input up to witness v0, its scriptPubKey and amount handed in by the
// caller) and bcc_taproot_spend_batch (taproot_spend.cpp: native v1 programs, the spent outputs of
// the whole transaction).  This file is the routing in front of them and nothing else: one pass
// over the items settles the contract's rules 1-3 (flags, the transaction errors, the spent
// outputs), finds spent[n_in] and deals every remaining item to one of the two entries, which are
// called as they are; their answers are scattered back by index into one (ret, err) convention.
//
// The routing pass runs on the calling thread's team in contiguous slices.  A slice keeps the
// parsed transaction and the parsed spent outputs of its current run of items (same tx and
// spent_outputs pointers and lengths), so the compact sizes of a 442-input transaction's outputs
// are walked once per slice, not once per input.  Each slice appends to its own lists; the lists
// are concatenated in slice order, so the partition is stable and adjacent inputs of one
// transaction stay adjacent on their side (both entries share per-tx work between such items).
//
// When both sides have items they run at the same time: the ECDSA subset on the calling thread, the
// Taproot subset on a second thread the calling thread keeps (SideWorker).  Teams and device state
// belong to the thread that calls an entry (team.h, bcc_release_thread_state), so the second thread
// is simply a concurrent caller; each side's host pass fills the time the other waits for its
// device rounds.  Measured against running the sides one after the other: DESIGN.md 3.14.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "bcc_amd.h"
#include "devices.h"
#include "inputs.h"
#include "taproot_host.h"
#include "team.h"
#include "tuples.h"
#include "tx.h"

namespace bcc {
namespace host {
namespace {

using clk = std::chrono::steady_clock;
double since(clk::time_point t0) { return std::chrono::duration<double>(clk::now() - t0).count(); }

thread_local bcc_inputs_stats t_inputs_stats;

// The calling thread's second caller: a persistent thread, parked between calls, with the team and
// the device state every calling thread gets.  Joined when the calling thread exits or releases
// its state.
class SideWorker {
public:
    SideWorker() : th_([this] { loop(); }) {}
    ~SideWorker() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        th_.join();
    }
    void start(std::function<void()> job) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            job_ = std::move(job);
            busy_ = true;
        }
        cv_.notify_all();
    }
    void wait() {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [this] { return !busy_; });
    }

private:
    void loop() {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [this] { return stop_ || (busy_ && job_); });
            if (stop_) return;
            auto job = std::move(job_);
            job_ = nullptr;
            lk.unlock();
            job();
            lk.lock();
            busy_ = false;
            cv_.notify_all();
        }
    }
    std::mutex mu_;
    std::condition_variable cv_;
    std::function<void()> job_;
    bool busy_ = false, stop_ = false;
    std::thread th_;
};
thread_local std::unique_ptr<SideWorker> tl_side;

// One slice's share of the two sides: the items in order, and where each came from.
struct alignas(64) RoutePart {
    std::vector<bcc_batch_item> ecdsa;
    std::vector<bcc_taproot_spend> taproot;
    std::vector<size_t> ecdsa_idx, taproot_idx;
    size_t host_decided = 0;
};

// The transaction and the spent outputs a run of adjacent items shares.
struct Run {
    const uint8_t* tx = nullptr;
    const uint8_t* spent = nullptr;
    unsigned tx_len = 0, spent_len = 0;
    bool tx_ok = false, spent_ok = false;
    Tx t;
    std::vector<TxOut> outs;
};

void load_run(Run& r, const bcc_input& it) {
    if (r.tx == it.tx && r.tx_len == it.tx_len && r.spent == it.spent_outputs &&
        r.spent_len == it.spent_outputs_len)
        return;
    r.tx = it.tx;
    r.tx_len = it.tx_len;
    r.spent = it.spent_outputs;
    r.spent_len = it.spent_outputs_len;
    try {
        r.tx_ok = parse_tx(it.tx, it.tx_len, r.t);
    } catch (...) {
        r.tx_ok = false;
    }
    try {
        r.spent_ok = r.tx_ok && parse_txouts(it.spent_outputs, it.spent_outputs_len, r.outs) &&
                     r.outs.size() == r.t.vin.size();
    } catch (...) {
        r.spent_ok = false;
    }
}

// Items [lo, hi): rules 2 and 3 written to ret / err where they decide, every other item onto its
// side.
void route(const bcc_input* items, size_t lo, size_t hi, bool taproot, int* ret, int* err,
           RoutePart& P) {
    P.ecdsa.clear();
    P.taproot.clear();
    P.ecdsa_idx.clear();
    P.taproot_idx.clear();
    P.host_decided = 0;
    Run r;
    for (size_t i = lo; i < hi; i++) {
        const bcc_input& it = items[i];
        load_run(r, it);
        // rule 2, in the order of bitcoinconsensus.cpp:79-102 (the engine's: deserialize, nIn, size)
        int e = bitcoinconsensus_ERR_OK;
        if (!r.tx_ok) e = bitcoinconsensus_ERR_TX_DESERIALIZE;
        else if (it.n_in >= r.t.vin.size()) e = bitcoinconsensus_ERR_TX_INDEX;
        else if (r.t.ser_size != it.tx_len) e = bitcoinconsensus_ERR_TX_SIZE_MISMATCH;
        else if (!r.spent_ok) e = BCC_ERR_SPENT_OUTPUTS_MISMATCH;  // rule 3
        if (e != bitcoinconsensus_ERR_OK) {
            ret[i] = 0;
            if (err) err[i] = e;
            P.host_decided++;
            continue;
        }
        const TxOut& o = r.outs[it.n_in];
        if (taproot && o.script.n == 34 && o.script.p[0] == 0x51 && o.script.p[1] == 0x20) {
            P.taproot.push_back(it);
            P.taproot_idx.push_back(i);
        } else {
            P.ecdsa.push_back(bcc_batch_item{o.script.p, (unsigned)o.script.n, o.value, it.tx,
                                             it.tx_len, it.n_in});
            P.ecdsa_idx.push_back(i);
        }
    }
}

template <class T>
void append(std::vector<T>& dst, size_t at, const std::vector<T>& src) {
    if (!src.empty()) memcpy(dst.data() + at, src.data(), src.size() * sizeof(T));
}

bool flags_accepted(unsigned flags) {
    const unsigned all = bitcoinconsensus_SCRIPT_FLAGS_VERIFY_ALL;
    if (flags & BCC_SCRIPT_FLAGS_VERIFY_TAPROOT) return flags == (all | BCC_SCRIPT_FLAGS_VERIFY_TAPROOT);
    return (flags & ~all) == 0;
}

long run_inputs(const bcc_input* items, size_t n, unsigned flags, int* ret_out, int* err_out) {
    bcc_inputs_stats& st = t_inputs_stats;
    st = bcc_inputs_stats{};
    st.items = n;
    const auto t0 = clk::now();
    if (!flags_accepted(flags)) {  // rule 1
        for (size_t i = 0; i < n; i++) {
            ret_out[i] = 0;
            if (err_out) err_out[i] = bitcoinconsensus_ERR_INVALID_FLAGS;
        }
        st.host_decided_items = n;
        st.total_seconds = since(t0);
        return 0;
    }
    const bool taproot = (flags & BCC_SCRIPT_FLAGS_VERIFY_TAPROOT) != 0;
    const unsigned base = flags & ~(unsigned)BCC_SCRIPT_FLAGS_VERIFY_TAPROOT;

    const unsigned T = pool_threads(n, 1024);
    std::vector<RoutePart> parts(T);
    run_team(T, [&](unsigned t) {
        route(items, n * t / T, n * (t + 1) / T, taproot, ret_out, err_out, parts[t]);
    });
    std::vector<size_t> e0(T + 1, 0), p0(T + 1, 0);
    for (unsigned t = 0; t < T; t++) {
        e0[t + 1] = e0[t] + parts[t].ecdsa.size();
        p0[t + 1] = p0[t] + parts[t].taproot.size();
        st.host_decided_items += parts[t].host_decided;
    }
    const size_t ne = e0[T], np = p0[T];
    std::vector<bcc_batch_item> ecdsa(ne);
    std::vector<bcc_taproot_spend> spends(np);
    std::vector<size_t> ecdsa_idx(ne), spend_idx(np);
    run_team(T, [&](unsigned t) {
        append(ecdsa, e0[t], parts[t].ecdsa);
        append(ecdsa_idx, e0[t], parts[t].ecdsa_idx);
        append(spends, p0[t], parts[t].taproot);
        append(spend_idx, p0[t], parts[t].taproot_idx);
        parts[t] = RoutePart();
    });
    st.ecdsa_side_items = ne;
    st.taproot_side_items = np;
    st.route_seconds = since(t0);

    long status = 0, valid = 0;
    std::vector<int> r, e;
    // One v1 item's answer: VerifyScript's verdict, or, where a failed device round left none
    // (BCC_DEVICE_FAILURE_ERROR), ret 0 / BCC_ERR_DEVICE_FAILURE as the other side reports it.
    auto scatter_spend = [&](size_t i, int ret, uint8_t no_verdict) {
        ret_out[i] = !no_verdict && ret == 1 ? 1 : 0;
        if (err_out) err_out[i] = no_verdict ? BCC_ERR_DEVICE_FAILURE : bitcoinconsensus_ERR_OK;
        valid += !no_verdict && ret == 1;
    };
    if (ne && np) {
        const auto t1 = clk::now();
        std::vector<int> rt(np), et(np);
        std::vector<uint8_t> unfinished(np, 0);
        r.resize(ne);
        e.resize(ne);
        int rc_t = 0;
        double taproot_s = 0;
        bcc_taproot_stats side_stats{};
        if (!tl_side) tl_side.reset(new SideWorker());
        tl_side->start([&] {
            const auto t2 = clk::now();
            rc_t = taproot_spend_run(spends.data(), np, rt.data(), et.data(), -1, unfinished.data());
            bcc_last_taproot_stats(&side_stats);  // that thread's last call: handed to the caller
            taproot_s = since(t2);
        });
        long rc = -1;
        try {
            rc = bitcoinconsensus_verify_batch(ecdsa.data(), ne, base, r.data(),
                                               reinterpret_cast<bitcoinconsensus_error*>(e.data()));
        } catch (...) {
        }
        st.ecdsa_side_seconds = since(t1);
        tl_side->wait();  // (before anything the job refers to leaves scope)
        st.taproot_side_seconds = taproot_s;
        taproot_stats_set(side_stats);
        if (rc < 0 || rc_t != 0) status = -1;
        // (rule 2 passed, so err is OK, or BCC_ERR_DEVICE_FAILURE where the device left no verdict)
        for (size_t k = 0; k < ne; k++) {
            ret_out[ecdsa_idx[k]] = r[k];
            if (err_out) err_out[ecdsa_idx[k]] = e[k];
            valid += r[k] == 1;
        }
        // ret -1 after rules 1-3: a scriptSig whose result hangs on ECDSA verdicts.  It is invalid
        // under every verdict (its own script error, or WITNESS_MALLEATED), and the script error is
        // not part of this contract.
        for (size_t k = 0; k < np; k++) scatter_spend(spend_idx[k], rt[k], unfinished[k]);
        st.total_seconds = since(t0);
        return status < 0 ? -1 : valid;
    }
    // one side only: on the calling thread
    if (ne) {
        const auto t1 = clk::now();
        r.resize(ne);
        e.resize(ne);
        const long rc = bitcoinconsensus_verify_batch(ecdsa.data(), ne, base, r.data(),
                                                      reinterpret_cast<bitcoinconsensus_error*>(e.data()));
        if (rc < 0) status = -1;
        for (size_t k = 0; k < ne; k++) {
            ret_out[ecdsa_idx[k]] = r[k];
            if (err_out) err_out[ecdsa_idx[k]] = e[k];
            valid += r[k] == 1;
        }
        st.ecdsa_side_seconds = since(t1);
    }
    if (np) {
        const auto t1 = clk::now();
        r.resize(np);
        e.resize(np);
        std::vector<uint8_t> unfinished(np, 0);
        if (taproot_spend_run(spends.data(), np, r.data(), e.data(), -1, unfinished.data()) != 0)
            status = -1;
        for (size_t k = 0; k < np; k++) scatter_spend(spend_idx[k], r[k], unfinished[k]);  // (ret -1: see above)
        st.taproot_side_seconds = since(t1);
    }
    st.total_seconds = since(t0);
    return status < 0 ? -1 : valid;
}

}  // namespace

void inputs_release_thread_state() {
    if (!tl_side) return;
    tl_side->start([] { bcc_release_thread_state(); });  // the second caller's own state, on its thread
    tl_side->wait();
    tl_side.reset();
}

}  // namespace host
}  // namespace bcc

extern "C" {

long bcc_verify_inputs_batch(const bcc_input* items, size_t n, unsigned int flags, int* ret_out,
                             int* err_out) {
    if (n == 0) {
        bcc::host::t_inputs_stats = bcc_inputs_stats{};
        return 0;
    }
    if (!items || !ret_out) return -1;
    for (size_t i = 0; i < n; i++)
        if (!items[i].tx || !items[i].spent_outputs) return -1;
    bcc::host::ActiveCaller active;
    try {
        return bcc::host::run_inputs(items, n, flags, ret_out, err_out);
    } catch (...) {
        return -1;
    }
}

int bcc_verify_input(const unsigned char* tx, unsigned int tx_len, const unsigned char* spent_outputs,
                     unsigned int spent_outputs_len, unsigned int n_in, unsigned int flags, int* err) {
    // a null buffer is an empty one: it then fails rule 2 or rule 3 like any other
    static const unsigned char none = 0;
    const bcc_input item{tx ? tx : &none, tx ? tx_len : 0u, spent_outputs ? spent_outputs : &none,
                         spent_outputs ? spent_outputs_len : 0u, n_in};
    int ret = 0, e = bitcoinconsensus_ERR_OK;
    if (bcc_verify_inputs_batch(&item, 1, flags, &ret, &e) < 0) {
        // no verdict (a failed device round under BCC_DEVICE_FAILURE_ERROR; the default policy
        // verifies such a round on the host CPU): as bitcoinconsensus_verify_script_with_amount,
        // the single-item call has no code for it and must not report a consensus failure
        fprintf(stderr, "[bcc] bcc_verify_input: GPU unavailable, no verdict; aborting\n");
        abort();
    }
    if (err) *err = e;
    return ret;
}

void bcc_last_inputs_stats(bcc_inputs_stats* out) {
    if (out) *out = bcc::host::t_inputs_stats;
}

}  // extern "C"
