// Whole Taproot inputs in batch: bcc_taproot_spend_batch (include/bcc_amd.h).
//
// The host pass restates VerifyScript for a native v1 program (interpreter.cpp:1937-2056) and
// VerifyWitnessProgram's v1 branch (:1889-1927): the annex, the key path, the control-size rule,
// the leaf version, and for 0xc0 one interpreter run of the tapscript (script.cpp
// execute_tapscript) with a deferring checker.  In BIP342 a signature opcode with a non-empty
// signature either verifies or fails the whole script, so a run never depends on a verdict: the
// checker applies the size / hash_type rules, answers true and records the check, and no script
// runs twice.  What is left for the device per round: the script-path commitments (which also
// yield the TapLeaf hashes the recorded checks' signature hashes need) and every signature check,
// key path and tapscript together.  The device round is reached through g_spend_device_hook
// (taproot_spend.h); without one, round_host composes the commitment lane code (taproot_commit.h)
// with gpu_taproot_verify_parts.  A small round, and a round the device could not deliver, runs on
// the host CPU altogether: the same lane code and host_taproot_parts (taproot_host.h).
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "bcc_amd.h"
#include "devices.h"
#include "host_verify.h"
#include "script.h"
#include "taproot_commit.h"
#include "taproot_host.h"
#include "taproot_jobs.h"
#include "taproot_spend.h"
#include "team.h"
#include "tuples.h"

namespace bcc {

const SpendDeviceHook* g_spend_device_hook = nullptr;

namespace host {
namespace {

constexpr int SCRIPT_ERR_UNKNOWN_ERROR = 1;
constexpr uint8_t ANNEX_TAG = 0x50, TAPROOT_LEAF_MASK = 0xfe, TAPROOT_LEAF_TAPSCRIPT = 0xc0;
constexpr size_t SPEND_ROUND_DEFAULT = 65536;
std::atomic<size_t> g_spend_round{0};

// One part's bookkeeping beside its SpendPart: which item a row / a commitment belongs to.
struct alignas(64) PartMeta {
    std::vector<uint32_t> item_of_row, item_of_commit;
};

// A launched round: its rows' and commitments' items (parts concatenated) and the verdict buffers.
struct RoundOut {
    std::vector<uint32_t> item_of_row, item_of_commit;
    std::vector<uint8_t> sig_verdict, commit_verdict;
};

// ::GetSerializeSize(witness.stack) (interpreter.cpp:1918)
size_t witness_serialized_size(const std::vector<Span>& w) {
    auto cs = [](size_t n) { return n < 253 ? (size_t)1 : n <= 0xFFFF ? (size_t)3 : (size_t)5; };
    size_t s = cs(w.size());
    for (const Span& e : w) s += cs(e.n) + e.n;
    return s;
}

// The checker of a non-empty scriptSig's run (SIGVERSION_BASE).  This entry has no ECDSA lane, so
// it answers every check of a non-empty signature with `answer` and counts them; an empty
// signature fails as in the reference.
class ScriptSigChecker : public SigChecker {
public:
    ScriptSigChecker(const Tx& t, unsigned nin, bool answer) : t_(t), nin_(nin), answer_(answer) {}
    bool check_ecdsa(const Bytes& sig, const Bytes&, const Bytes&, SigVersion) override {
        if (sig.empty()) return false;
        assumed++;
        return answer_;
    }
    bool check_locktime(int64_t n) override { return tx_check_locktime(t_, nin_, n); }
    bool check_sequence(int64_t n) override { return tx_check_sequence(t_, nin_, n); }
    int assumed = 0;

private:
    const Tx& t_;
    unsigned nin_;
    bool answer_;
};

// The deferring checker of a tapscript run.
class SpendChecker : public SigChecker {
public:
    SpendChecker(TxState& s, SpendPart& part, PartMeta& meta, uint32_t item, unsigned nin,
                 const Span* annex, uint32_t lane, std::vector<uint8_t>& scratch)
        : s_(s), part_(part), meta_(meta), item_(item), nin_(nin), annex_(annex), lane_(lane),
          scratch_(scratch) {}
    bool check_ecdsa(const Bytes&, const Bytes&, const Bytes&, SigVersion) override { return false; }
    bool check_schnorr(const Bytes& sig, const uint8_t* key32, uint32_t codesep_pos) override {
        uint32_t slot = 0;
        const int e = taproot_add_check(s_, part_.jobs, nin_, sig.data(), (unsigned)sig.size(), key32,
                                        true, annex_ ? annex_->p : nullptr,
                                        annex_ ? (unsigned)annex_->n : 0u, nullptr, codesep_pos,
                                        scratch_, &slot);
        if (e) {
            err_ = e == BCC_SCRIPT_ERR_SCHNORR_SIG_SIZE ? SERR_SCHNORR_SIG_SIZE : SERR_SCHNORR_SIG_HASHTYPE;
            return false;
        }
        meta_.item_of_row.push_back(item_);
        part_.copies.push_back(LeafCopy{lane_, slot});
        return true;
    }
    ScriptErr schnorr_error() const override { return err_; }
    bool check_locktime(int64_t n) override { return tx_check_locktime(s_.t, nin_, n); }
    bool check_sequence(int64_t n) override { return tx_check_sequence(s_.t, nin_, n); }

private:
    TxState& s_;
    SpendPart& part_;
    PartMeta& meta_;
    uint32_t item_;
    unsigned nin_;
    const Span* annex_;
    uint32_t lane_;
    std::vector<uint8_t>& scratch_;
    ScriptErr err_ = SERR_SCHNORR_SIG;
};

// Items [lo, hi): everything VerifyScript decides without a hash of the tx or a curve operation;
// ret / serr receive the final result, or for an item with device work the result it has when
// that work passes.
void build_part(const bcc_taproot_spend* items, size_t lo, size_t hi, int* ret, int* serr,
                SpendPart& P, PartMeta& M) {
    P.jobs.clear();
    P.copies.clear();
    P.commits.clear();
    M.item_of_row.clear();
    M.item_of_commit.clear();
    TxState s;
    std::vector<uint8_t> scratch;
    for (size_t i = lo; i < hi; i++) {
        const bcc_taproot_spend& it = items[i];
        auto set = [&](int r, int e) {
            ret[i] = r;
            serr[i] = e;
        };
        // (BIP341-readiness needs no test: a signature check is reached only by a non-empty
        // witness on this 34-byte OP_1 output, which is what makes the tx data ready)
        load_tx(s, it.tx, it.tx_len, it.spent_outputs, it.spent_outputs_len);
        if (!s.parsed || it.n_in >= s.t.vin.size()) {
            set(-1, SCRIPT_ERR_UNKNOWN_ERROR);
            continue;
        }
        const TxIn& in = s.t.vin[it.n_in];
        const Span spk = s.outs[it.n_in].script;
        if (spk.n != 34 || spk.p[0] != 0x51 || spk.p[1] != 0x20) {
            set(-1, SCRIPT_ERR_UNKNOWN_ERROR);
            continue;
        }
        const uint8_t* program = spk.p + 2;
        if (in.script_sig.n != 0) {
            // VerifyScript runs the scriptSig and the scriptPubKey first; what survives both is
            // WITNESS_MALLEATED (v1 passes unchecked in verify_script, so it reports exactly the
            // failures that come before the witness program)
            // A check of a non-empty signature cannot be verified here.  The script is run with
            // the answer false and, if that run met such a check, again with true: with no check
            // the first run is the result; with exactly one check in both runs the two runs cover
            // both verdicts, so an equal result is the result whatever the verdict.  Else ret -1.
            int code[2] = {0, 0}, assumed[2] = {0, 0};
            for (int pass = 0; pass < 2; pass++) {
                ScriptSigChecker chk(s.t, it.n_in, pass == 1);
                ScriptErr se = SERR_UNKNOWN;
                bool ok = false;
                try {
                    ok = verify_script(in.script_sig, spk, in.witness, FLAGS_VERIFY_ALL, chk, &se);
                } catch (...) {
                    ok = false;
                    se = SERR_UNKNOWN;
                }
                code[pass] = script_err_code(ok ? SERR_WITNESS_MALLEATED : se);
                assumed[pass] = chk.assumed;
                if (chk.assumed == 0) break;
            }
            if (assumed[0] == 0) set(0, code[0]);
            else if (assumed[0] == 1 && assumed[1] == 1 && code[0] == code[1]) set(0, code[0]);
            else set(-1, SCRIPT_ERR_UNKNOWN_ERROR);
            continue;
        }
        // the scriptPubKey leaves <1> <program>: the program is the truth value
        if (!cast_to_bool(program, 32)) {
            set(0, BCC_SCRIPT_ERR_EVAL_FALSE);
            continue;
        }
        // VerifyWitnessProgram, v1, 32 bytes, not P2SH-wrapped (interpreter.cpp:1889-1927)
        size_t nw = in.witness.size();
        if (nw == 0) {
            set(0, BCC_SCRIPT_ERR_WITNESS_PROGRAM_WITNESS_EMPTY);
            continue;
        }
        const Span* annex = nullptr;
        if (nw >= 2 && in.witness[nw - 1].n != 0 && in.witness[nw - 1].p[0] == ANNEX_TAG) {
            annex = &in.witness[nw - 1];
            nw--;
        }
        if (nw == 1) {  // key path
            const Span& sig = in.witness[0];
            const int e = taproot_add_check(s, P.jobs, it.n_in, sig.p, (unsigned)sig.n, program, false,
                                            annex ? annex->p : nullptr, annex ? (unsigned)annex->n : 0u,
                                            nullptr, 0, scratch);
            if (e) {
                set(0, e);
                continue;
            }
            M.item_of_row.push_back((uint32_t)i);
            set(1, 0);
            continue;
        }
        const Span& control = in.witness[nw - 1];
        const Span& script = in.witness[nw - 2];
        if (!commit_control_size_ok((unsigned)control.n) || control.n > 0xFFFFFFFFu) {
            set(0, BCC_SCRIPT_ERR_TAPROOT_WRONG_CONTROL_SIZE);
            continue;
        }
        const uint32_t lane = (uint32_t)P.commits.size();
        P.commits.push_back(bcc_taproot_commit{control.p, (unsigned)control.n, script.p,
                                               (unsigned)script.n, program});
        M.item_of_commit.push_back((uint32_t)i);
        if ((control.p[0] & TAPROOT_LEAF_MASK) != TAPROOT_LEAF_TAPSCRIPT) {
            set(1, 0);  // an unknown leaf version: the commitment alone decides
            continue;
        }
        TapscriptData ex;
        ex.validation_weight_left = (int64_t)witness_serialized_size(in.witness) + 50;
        ScriptErr se = SERR_UNKNOWN;
        bool ok = false;
        try {
            std::vector<Bytes> stack;
            stack.reserve(nw + 2);
            for (size_t k = 0; k + 2 < nw; k++)
                stack.emplace_back(in.witness[k].p, in.witness[k].p + in.witness[k].n);
            SpendChecker chk(s, P, M, (uint32_t)i, it.n_in, annex, lane, scratch);
            ok = execute_tapscript(std::move(stack), script, ex, chk, &se);
        } catch (...) {
            ok = false;
            se = SERR_UNKNOWN;
        }
        set(ok ? 1 : 0, ok ? 0 : script_err_code(se));
    }
}

const GCombArray host_comb() { return GCombArray{static_cast<const fe*>(host_comb_tables())}; }

// A round without the fused device path: every commitment on the host lanes (the kernels' lane
// code), the TapLeaf hashes copied into the checks' slots, then the signature parts: on the host
// too (sigs_on_host: a small round, or a round the device could not deliver), or through the
// device seam the engine has always had (a build without the fused round).
int round_host(int device, const SpendRound& R, uint8_t* commit_verdict, uint8_t* sig_verdict,
               bool sigs_on_host) {
    static const CommitMids mids = commit_mids();
    const GCombArray gc = host_comb();
    std::vector<size_t> c0(R.P + 1, 0);
    size_t rows = 0;
    for (size_t q = 0; q < R.P; q++) {
        c0[q + 1] = c0[q] + R.parts[q]->commits.size();
        rows += R.parts[q]->jobs.rows();
    }
    run_team((unsigned)R.P, [&](unsigned q) {
        SpendPart& S = *R.parts[q];
        const size_t n = S.commits.size();
        if (n == 0) return;
        std::vector<CommitLane> lanes(n);
        size_t lb = 0, nd = 0;
        commit_plan(S.commits.data(), n, lanes.data(), &lb, &nd);
        // u32-aligned rows: p | q | nodes | leaf | parity, then the leaf hashes
        std::vector<u32> buf((64 * n + 32 * nd + 64 * lb + n + 3) / 4 + 1), leafh(8 * n);
        uint8_t* b = reinterpret_cast<uint8_t*>(buf.data());
        uint8_t *p = b, *qq = b + 32 * n, *nodes = qq + 32 * n, *leaf = nodes + 32 * nd,
                *par = leaf + 64 * lb;
        uint8_t* lh = reinterpret_cast<uint8_t*>(leafh.data());
        commit_fill(S.commits.data(), lanes.data(), 0, n, p, qq, par, nodes, leaf);
        for (size_t i = 0; i < n; i++) {
            int r = 0, e = 0;
            commit_host_lane(mids, lanes.data(), i, p, qq, par, nodes, leaf, gc, &r, &e, lh + 32 * i);
            commit_verdict[c0[q] + i] = (uint8_t)(r == 1);
        }
        for (const LeafCopy& c : S.copies) memcpy(&S.jobs.dev.ext[c.ext_byte], lh + 32 * c.lane, 32);
    });
    if (rows == 0) return 0;
    std::vector<const TaprootJobs*> pj;
    for (size_t q = 0; q < R.P; q++) pj.push_back(&R.parts[q]->jobs);
    if (sigs_on_host) {
        host_taproot_parts(pj.data(), pj.size(), sig_verdict, nullptr, host_threads());
        return 0;
    }
    return gpu_taproot_verify_parts(device, pj.data(), pj.size(), sig_verdict, nullptr);
}

// The round's verdicts onto its items: a commitment mismatch first, then a failed signature check,
// else what the host pass left.
void apply_round(const RoundOut& o, int* ret, int* serr) {
    for (size_t c = 0; c < o.item_of_commit.size(); c++)
        if (!o.commit_verdict[c]) {
            ret[o.item_of_commit[c]] = 0;
            serr[o.item_of_commit[c]] = BCC_SCRIPT_ERR_WITNESS_PROGRAM_MISMATCH;
        }
    for (size_t r = 0; r < o.item_of_row.size(); r++) {
        const uint32_t i = o.item_of_row[r];
        if (!o.sig_verdict[r] && serr[i] != BCC_SCRIPT_ERR_WITNESS_PROGRAM_MISMATCH) {
            ret[i] = 0;
            serr[i] = BCC_SCRIPT_ERR_SCHNORR_SIG;
        }
    }
}

// Items [lo, hi) on `device` in rounds that rotate over the Taproot contexts: round k's host pass
// runs while rounds k - 1 and k - 2 are on the GPU, and its upload beside their kernels.  A round of
// at most host_small_round() checks (signature rows + commitments) runs on the host and touches no
// device state.  A round the device cannot deliver (an injected fault, a failed begin or end) is
// rebuilt from its items, re-run once if the error is transient, and else left to the failure
// policy: verified on the host, or (BCC_DEVICE_FAILURE_ERROR) its items marked in `unfinished`
// (optional, one byte per item) together with every item of the range not yet decided.
int run_range(const bcc_taproot_spend* items, size_t lo, size_t hi, int* ret, int* serr, int device,
              TaprootCounters& c, uint8_t* unfinished) {
    constexpr const char* WHO = "taproot_spend_batch";
    const SpendDeviceHook* hook = g_spend_device_hook;
    const size_t set_round = g_spend_round.load(std::memory_order_relaxed);
    const size_t RS = set_round ? set_round : SPEND_ROUND_DEFAULT;
    std::vector<SpendPart> parts;
    std::vector<PartMeta> metas;
    std::vector<SpendPart*> pp;
    RoundOut outs[TAPROOT_SLOTS];
    struct Flight {
        int slot;
        size_t lo, hi;  // its item range: a failed round is rebuilt from it
    };
    std::vector<Flight> inflight;
    DeviceRange fail;
    int err = 0;
    // The host pass of items [a, b) into parts / metas, and the round's item maps and verdict
    // buffers into o.  Returns 0 (no device work), 1, or -1 (blobs beyond the 32-bit offsets).
    auto build = [&](size_t a, size_t b, RoundOut& o) -> int {
        const unsigned T = pool_threads(b - a, 1024);
        if (parts.size() < T) {
            parts.resize(T);
            metas.resize(T);
        }
        run_team(T, [&](unsigned t) {
            build_part(items, a + (b - a) * t / T, a + (b - a) * (t + 1) / T, ret, serr, parts[t],
                       metas[t]);
        });
        size_t raw = 0, ext = 0;
        o.item_of_row.clear();
        o.item_of_commit.clear();
        pp.clear();
        for (unsigned t = 0; t < T; t++) {
            pp.push_back(&parts[t]);
            o.item_of_row.insert(o.item_of_row.end(), metas[t].item_of_row.begin(), metas[t].item_of_row.end());
            o.item_of_commit.insert(o.item_of_commit.end(), metas[t].item_of_commit.begin(),
                                    metas[t].item_of_commit.end());
            raw += parts[t].jobs.dev.txraw.size();
            ext += parts[t].jobs.dev.ext.size();
        }
        o.commit_verdict.assign(o.item_of_commit.size() + 1, 0);
        o.sig_verdict.assign(o.item_of_row.size() + 1, 0);
        if (o.item_of_row.empty() && o.item_of_commit.empty()) return 0;
        if (raw >= ((size_t)1 << 32) || ext >= ((size_t)1 << 32)) {
            fprintf(stderr, "[bcc] bcc_taproot_spend_batch: a round's blobs exceed 4 GiB; lower bcc_set_spend_round\n");
            return -1;
        }
        return 1;
    };
    auto give_up = [&](const RoundOut& o) {  // no verdict for this round's items
        if (!unfinished) return;
        for (uint32_t i : o.item_of_row) unfinished[i] = 1;
        for (uint32_t i : o.item_of_commit) unfinished[i] = 1;
    };
    auto on_host = [&](RoundOut& o) {  // the round in parts / o, all of it on the host CPU
        const SpendRound R{pp.data(), pp.size()};
        round_host(device, R, o.commit_verdict.data(), o.sig_verdict.data(), true);
        c.round(o.item_of_row.size(), o.item_of_commit.size(), true);
        apply_round(o, ret, serr);
    };
    // Round f failed with e at its begin (parts still hold its own host pass) or at its end (by
    // then they hold a later round's, so the round is rebuilt from its items: the pass is
    // deterministic).
    auto recover = [&](const Flight& f, int e, bool parts_intact) -> int {
        RoundOut& o = outs[f.slot];
        FailedRound r;
        if (!parts_intact) r.rebuild = [&] { build(f.lo, f.hi, o); };
        r.checks = [&] { return o.item_of_row.size() + o.item_of_commit.size(); };
        r.run = [&] {
            const SpendRound R{pp.data(), pp.size()};
            if (int e2 = hook->begin(device, f.slot, R)) return e2;
            return hook->end(device, f.slot, o.commit_verdict.data(), o.sig_verdict.data());
        };
        r.host = [&] {
            const SpendRound R{pp.data(), pp.size()};
            round_host(device, R, o.commit_verdict.data(), o.sig_verdict.data(), true);
        };
        r.done = [&](bool on_host) {
            c.round(o.item_of_row.size(), o.item_of_commit.size(), on_host);
            apply_round(o, ret, serr);
        };
        r.lost = [&] { give_up(o); };
        return recover_round(WHO, device, e, fail, c, r);
    };
    auto finish = [&](const Flight& f) -> int {
        RoundOut& o = outs[f.slot];
        if (int e = hook->end(device, f.slot, o.commit_verdict.data(), o.sig_verdict.data()))
            return recover(f, e, false);
        c.round(o.item_of_row.size(), o.item_of_commit.size(), false);
        apply_round(o, ret, serr);
        return 0;
    };
    // slots rotate by LAUNCHED rounds: at most TAPROOT_SLOTS - 1 are in flight after a launch, so
    // the next launch's slot is never one of them (a round without device work launches nothing
    // and must not advance the rotation)
    size_t launched = 0, a = lo;
    for (; a < hi && !err; a += RS) {
        const size_t b = std::min(hi, a + RS);
        const int slot = (int)(launched % TAPROOT_SLOTS);
        RoundOut& o = outs[slot];  // free: its last round was finished before two later launches
        const int work = build(a, b, o);
        if (work == 0) continue;  // decided on the host: no slot is touched
        if (work < 0) {
            give_up(o);
            err = -1;
            a += RS;
            break;
        }
        const SpendRound R{pp.data(), pp.size()};
        if (o.item_of_row.size() + o.item_of_commit.size() <= host_small_round()) {
            on_host(o);
            continue;
        }
        if (!hook) {  // (a build without the fused round: commitment lanes + the signature seam)
            err = resilient_taproot_round(WHO, device, o.item_of_row.size(), o.item_of_commit.size(),
                                          fail, c, [&] {
                return round_host(device, R, o.commit_verdict.data(), o.sig_verdict.data(), false);
            }, [&] {
                round_host(device, R, o.commit_verdict.data(), o.sig_verdict.data(), true);
            });
            if (!err) apply_round(o, ret, serr);
            else give_up(o);
            continue;
        }
        // an injected fault, or an earlier error that left the context unusable, comes before the
        // launch: such a round never reaches the GPU
        const Flight f{slot, a, b};
        int e = round_blocked(fail);
        if (!e) e = hook->begin(device, slot, R);
        if (e) {
            err = recover(f, e, true);
        } else {
            inflight.push_back(f);
            launched++;
        }
        while ((int)inflight.size() > TAPROOT_SLOTS - 1 || (err && !inflight.empty())) {
            const Flight p = inflight.front();
            inflight.erase(inflight.begin());
            const int e2 = finish(p);
            if (!err) err = e2;
        }
    }
    for (const Flight& f : inflight) {  // in launch order; every launched round is ended, even after an error
        const int e = finish(f);
        if (!err) err = e;
    }
    if (err) {
        fprintf(stderr, "[bcc] bcc_taproot_spend_batch failed on device %d: %d\n", device, err);
        if (unfinished)
            for (size_t i = std::min(a, hi); i < hi; i++) unfinished[i] = 1;  // never built
    }
    return err;
}

}  // namespace

int taproot_spend_run(const bcc_taproot_spend* items, size_t n, int* ret_out, int* serror_out,
                      int device, uint8_t* unfinished) {
    if (n == 0) return 0;
    if (!items || !ret_out || !serror_out) return -1;
    for (size_t i = 0; i < n; i++)
        if (!items[i].tx || !items[i].spent_outputs) return -1;
    if (unfinished) memset(unfinished, 0, n);
    ActiveCaller active;
    std::vector<int> devs = device < 0 ? device_list() : std::vector<int>{device};
    const size_t D = std::max<size_t>(1, std::min<size_t>(devs.size(), (n + 4095) / 4096));
    devs.resize(D);
    TaprootCounters counters;
    std::vector<std::function<int()>> jobs;
    for (size_t d = 0; d < D; d++) {
        const size_t lo = n * d / D, hi = n * (d + 1) / D;
        const int dev = devs[d];
        jobs.push_back([=, &counters] {
            return run_range(items, lo, hi, ret_out, serror_out, dev, counters, unfinished);
        });
    }
    const int rc = run_on_devices(devs, jobs);
    taproot_stats_store(n, counters);
    return rc ? -1 : 0;
}

}  // namespace host
}  // namespace bcc

extern "C" int bcc_set_spend_round(size_t items) {
    bcc::host::g_spend_round.store(items, std::memory_order_relaxed);
    return 0;
}

extern "C" int bcc_taproot_spend_batch(const bcc_taproot_spend* items, size_t n, int* ret_out,
                                       int* serror_out, int device) {
    return bcc::host::taproot_spend_run(items, n, ret_out, serror_out, device, nullptr);
}
