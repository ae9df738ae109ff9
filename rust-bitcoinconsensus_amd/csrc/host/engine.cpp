// The drop-in C ABI (include/bitcoinconsensus.h) and the batch engine behind it.
//
// verify_script semantics (script/bitcoinconsensus.cpp:79-102): flags -> deserialize -> nIn ->
// size -> ERR_OK -> VerifyScript.  VerifyScript runs on the host (script.cpp) with a DEFERRING
// checker: every CHECKSIG / CHECKMULTISIG pair is recorded as a GPU tuple and answered
// speculatively with `true`.  After the GPU round (sighash kernels + ECDSA kernel) an item whose
// deferred checks all came back true is final (its speculative run WAS the reference run);
// otherwise it is re-run with the verdicts learned so far, deferring only the checks it has not
// seen (e.g. the next multisig key), until a run needs no unknown verdict.  This reproduces the
// reference's verdict-dependent control flow (CHECKMULTISIG key advance, CHECKSIG NOT) exactly.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../pipeline.h"
#include "bcc_amd.h"
#include "bitcoinconsensus.h"
#include "devices.h"
#include "engine.h"
#include "hashes.h"
#include "host_verify.h"
#include "inputs.h"
#include "script.h"
#include "sighash.h"
#include "team.h"
#include "tuples.h"

namespace bcc {
namespace host {

namespace {
int g_device = -1;
std::mutex g_device_mu;
}  // namespace

int current_device() {
    std::lock_guard<std::mutex> lk(g_device_mu);
    if (g_device < 0) {
        const char* e = getenv("BCC_DEVICE");
        g_device = e ? atoi(e) : 0;
    }
    return g_device;
}

namespace {

thread_local bcc_batch_stats t_stats;
thread_local bcc_sighash_kinds t_kinds;  // bcc_last_sighash_kinds

// Fault injection (tests): the next N device rounds of any thread fail as if the HIP runtime had
// returned g_fail_code (bcc_debug_fail_device_rounds[_code], or BCC_FAULT_INJECT at load time).
std::atomic<int> g_fail_rounds{[] {
    const char* e = getenv("BCC_FAULT_INJECT");
    return e ? atoi(e) : 0;
}()};
std::atomic<int> g_fail_code{2};  // hipErrorOutOfMemory: transient

// A HIP error worth one retry on a fresh device batch: allocation / readiness trouble.  Anything
// else (launch failure, illegal address, no device, ECC, ...) leaves the context unusable, so the
// round goes straight to the failure policy.
bool retryable(int hip_error) {
    return hip_error == 2 /* hipErrorOutOfMemory */ || hip_error == 600 /* hipErrorNotReady */ ||
           hip_error == 1 /* hipErrorInvalidValue: staging limits */;
}

// Largest padded-message / template / code blob one device round may stage: the device job
// records address them with 32-bit byte offsets (pipeline.h PatchRec / TplJob).
constexpr size_t ROUND_BLOB_LIMIT = ((size_t)1 << 32) - ((size_t)1 << 24);

struct TxEntry {
    Tx tx;
    bool ok = false;
    int32_t aux[3] = {-1, -1, -1};  // aux message index per AuxKind in the current round
    int64_t tpl = -1;               // legacy template offset in the current round (-1: none)
    uint32_t tpl_len = 0;
    int32_t wtx = -1;               // WtxRec index in the current round (-1: none)
    uint32_t wtx_skip = 0;          // ... bytes of tx_to its upload leaves out after the version
                                    // (2: the segwit marker and flag), for offsets into it
    int64_t htpl = -1;              // host-kept legacy template offset (HostJobs::tpl), -1: none
    int32_t hdig = -1;              // host-computed BIP143 per-tx digests (HostJobs::dig), -1: none
    int64_t etpl = -1;              // legacy template offset in the shard's early jobs, -1: none
    uint32_t etpl_len = 0;          // ... its length (0: not measured yet this call)
};

// Long serial SHA chains stay on the host.  One GPU lane compresses one block
// in ~4 us (a lone wave issues the ~2,100 instructions of a template block one after another), the
// host's SHA extensions in ~35 ns.  A many-input transaction (block413567's 442-input tx) has
// chains of ~250-290 blocks -- its legacy preimages (every input's template is ~18 KB) and its
// BIP143 hashPrevouts -- which would set the whole device round's front at ~2 ms while the rest of
// the round's thousands of short chains finish in microseconds.  A check whose chain exceeds
// host_chain_blocks() blocks is therefore hashed on the host: BIP143 checks of such a tx inline
// (the per-tx digests once, then a ~4-block preimage each), legacy template / host-preimage jobs in
// a parallel pass over all shards (hash_host_jobs) that runs while the device round's
// message-independent kernels (K_inv, the key / Q-ladder launch, the sighash front) run; its
// digests reach the message rows just before the G ladder (LateHost, DeviceBatch::put_late).
// Legacy offload is for single-GPU rounds only (on several GPUs the pass would run before the
// round) and is capped per shard (HostJobs::BUDGET_BLOCKS).  Everything else is unchanged.
struct HostJobs {
    uint32_t chain_blocks = 0;       // legacy offload threshold in 64-byte blocks (0: never)
    uint32_t bip143_blocks = 0;      // BIP143 per-tx chain threshold (0: never)
    std::atomic<uint64_t>* planned = nullptr;  // legacy blocks sent to the host this pass, all shards
    std::vector<uint8_t> tpl, code;  // templates / code fields of offloaded legacy ALL jobs
    std::vector<TplJob> tjobs;       // offsets into tpl / code, row = the tuple row
    std::vector<uint8_t> pre;        // offloaded host preimages (NONE / SINGLE / ACP), unpadded
    std::vector<uint64_t> pre_off;   // pre_off[k] .. pre_off[k + 1]: preimage k
    std::vector<uint32_t> pre_row;
    std::vector<uint8_t> dig;        // 96 bytes per long BIP143 tx: prevouts / sequence / outputs
    size_t inline_rows = 0;          // rows whose msg add_sighash_job wrote itself
    size_t pending() const { return tjobs.size() + pre_row.size(); }
    void clear() {
        tpl.clear(); code.clear(); tjobs.clear(); pre.clear(); pre_off.assign(1, 0); pre_row.clear();
        dig.clear(); inline_rows = 0;
    }
    // Legacy work an interpreter pass may send to the host, in blocks, over all shards: the jobs
    // are hashed while the device round's message-independent kernels run (~1 ms), dealt over the
    // host threads at ~35 ns a block (2^19 blocks: ~1.1 ms on 16 threads, though a round's
    // chains above the default threshold are usually a fraction of it).  Beyond it the chains stay
    // on the GPU, whose lanes hash thousands of them side by side.
    static constexpr uint64_t BUDGET_BLOCKS = (uint64_t)1 << 19;
    bool take(uint64_t blocks) {
        if (!planned) return false;
        if (planned->fetch_add(blocks, std::memory_order_relaxed) + blocks <= BUDGET_BLOCKS)
            return true;
        planned->fetch_sub(blocks, std::memory_order_relaxed);
        return false;
    }
};

// A GPU lane hashes ~4 us a block, so a chain of more than ~200 blocks outlasts the device round's
// Q ladder (~0.9 ms for a small round) and would set the round's length.  Since round 5 the
// threshold applies to the blocks a job hashes from its template midstate (TPL_MID), i.e. only the
// first inputs of a many-input tx go to the host, at about half their former cost.
std::atomic<uint32_t> g_host_chain_blocks{[] {
    const char* e = getenv("BCC_HOST_CHAIN_BLOCKS");
    return e ? (uint32_t)atoi(e) : 160u;
}()};

// BIP143 checks of a tx whose hashPrevouts / hashSequence / hashOutputs chains exceed this many
// blocks are hashed on the host: the three per-tx digests once (one ~250-block chain for a
// 442-input tx: ~10 us on the host's SHA extensions, ~1.6 ms in one GPU lane), then a ~4-block
// preimage per check.  Unlike legacy preimages (O(inputs^2) bytes per tx) this is linear in the tx.
std::atomic<uint32_t> g_host_bip143_blocks{[] {
    const char* e = getenv("BCC_HOST_BIP143_BLOCKS");
    return e ? (uint32_t)atoi(e) : 32u;
}()};

// Key-hash spends (P2WPKH, P2PKH): the first run leaves HASH160(key) == program to the device,
// which checks it beside the signature (DeferringChecker::defer_key_hash, sighash.hip
// key_hash_kernel); prepare() then hashes nothing.  BCC_DEVICE_KEY_HASH=0 / bcc_set_device_key_hash(0):
// the host hashes every P2WPKH key in prepare() (the round-3 way).
std::atomic<bool> g_device_key_hash{[] {
    const char* e = getenv("BCC_DEVICE_KEY_HASH");
    return !(e && atoi(e) == 0);
}()};

// Device jobs for the remaining ECDSA-era hash types (bcc_set_device_hashtypes /
// BCC_DEVICE_HASHTYPES, default 0): legacy NONE / SINGLE / ANYONECANPAY checks become LinJobs and
// BIP143 SIGHASH_SINGLE checks WinJobs, both assembled on the device from the tx uploaded once per
// round, instead of one host-serialized preimage per check.  Results never depend on it.
std::atomic<bool> g_device_hashtypes{[] {
    const char* e = getenv("BCC_DEVICE_HASHTYPES");
    return e && atoi(e) != 0;
}()};

struct Item {
    const bcc_batch_item* in;
    TxEntry* tx = nullptr;
    int ret = 0;
    bitcoinconsensus_error err = bitcoinconsensus_ERR_OK;
    bool active = false;  // needs (another) interpreter run
    bool result = false;
    uint32_t runs = 0;    // interpreter runs so far in this call
    // checks seen by this item's runs: tuple key -> 0/1 known verdict, or -2 - r: deferred as
    // row r of the current round.  A flat list (an input makes a handful of checks, so a linear
    // scan beats a hash map); the key bytes live in the item's shard's key arena (Round::keys).
    struct Check {
        uint64_t off;  // into the shard's key arena (whole call: may exceed 4 GiB)
        uint32_t len;
        int32_t v;
    };
    std::vector<Check> cache;
    std::vector<uint32_t> pending;  // deferred rows the last run consulted (answered "true")
    // HASH160 of the P2WPKH witness key, computed ahead in a batch by prepare() (h160_src: the
    // hashed bytes; null when none)
    const uint8_t* h160_src = nullptr;
    uint32_t h160_len = 0;
    uint8_t h160[20];
    // early Q halves: this item's pre-extracted (key, signature) candidates in its shard's
    // EarlyShard::cands [ec_first, ec_first + ec_count)
    uint32_t ec_first = 0, ec_count = 0;
};

// Early Q halves (round 5).  A check's tuple row depends only on the bytes of its key and its
// signature, and K_keyq (the key half, u2 = r s^-1 and B = u2 Q) only on the row, so the rows of
// the standard spends (P2WPKH, P2PKH, P2SH-P2WPKH, P2SH multisig candidate pairs, P2PK) are
// pre-extracted right after deserialization and their K_keyq runs on the GPU while the host
// interprets (DeviceBatch::early_launch).  A row the interpreter defers with exactly those key and
// signature bytes is mapped to its early twin (TupleRows::emap), whose result K_keyq copies; the
// match is by bytes, so a pattern that guessed wrong only wastes an early lane.
struct EarlyCand {
    const uint8_t* pub;
    const uint8_t* sig;
    uint32_t publen, siglen;
    uint32_t row;  // in the shard's early rows
    // early sighash (legacy SIGHASH_ALL over a long template): the row's message is hashed in the
    // early set from this scriptCode; a deferred check with the same code bytes takes it (TPL_EARLY)
    const uint8_t* code = nullptr;
    uint32_t code_len = 0;
    bool msg = false;
};
struct alignas(64) EarlyShard {  // one per shard, written by its worker: own cache lines
    TupleRows rows;
    std::vector<EarlyCand> cands;
    SighashJobs jobs;  // the early sighash template jobs (rows: the early rows above)
    void clear() {
        rows.clear();
        rows.msg_one = true;
        rows.y_unused = true;
        cands.clear();
        jobs.clear();
    }
};

std::atomic<int> g_early_q{[] {
    const char* e = getenv("BCC_EARLY_Q");
    return e ? atoi(e) : 1;
}()};
constexpr size_t EARLY_MAX_ITEMS = (size_t)1 << 18;
// Per-shard row pre-upload for pipelined chunks (round 6, bcc_set_pre_upload / BCC_PRE_UPLOAD).
std::atomic<bool> g_pre_upload{[] {
    const char* e = getenv("BCC_PRE_UPLOAD");
    return !(e && atoi(e) == 0);
}()};
// early sighashes (BCC_EARLY_SIGHASH, default 1): legacy template jobs with the early rows.  Only
// the chains between BCC_EARLY_SIGHASH_MIN blocks (from the midstate) and the host's share
// (host_chain_blocks) go early: C3 5.4-5.7 -> 5.7-6.6 M inputs/s at 96 (64: 5.2-6.4; every long
// template, no cap: 4.9-5.2, the early chains then crowd the early K_keyq and duplicate the host's;
// profiles/r05/c3/early_sighash.txt).
const bool g_early_sighash = [] {
    const char* e = getenv("BCC_EARLY_SIGHASH");
    return e ? atoi(e) != 0 : true;
}();
// ... for jobs of at least this many blocks from their midstate (BCC_EARLY_SIGHASH_MIN)
const uint32_t g_early_sighash_min = [] {
    const char* e = getenv("BCC_EARLY_SIGHASH_MIN");
    return e ? (uint32_t)atoi(e) : 96u;
}();

// CPubKey size filter, non-empty signature, lax DER (sans the hash-type byte), r != 0, s != 0: the
// host half of a deferred check (Round::defer); false = rejected on the host, no row.
bool tuple_fields(const uint8_t* pub, size_t pl, const uint8_t* sig, size_t sl, uint8_t r[32],
                  uint8_t s[32]) {
    if (!pubkey_size_valid(pub, pl) || sl == 0 || !der_parse_lax(sig, sl - 1, r, s)) return false;
    uint64_t rw[4], sw[4];
    memcpy(rw, r, 32);
    memcpy(sw, s, 32);
    // secp256k1_ecdsa_sig_verify rejects r == 0 || s == 0
    return (rw[0] | rw[1] | rw[2] | rw[3]) != 0 && (sw[0] | sw[1] | sw[2] | sw[3]) != 0;
}

// The pushes of a push-only script (OP_0, direct pushes, PUSHDATA1 / 2), at most `cap`; -1 on any
// other opcode, a truncated push or more pushes.
int script_pushes(const Span& sc, Span* out, int cap) {
    const uint8_t* p = sc.p;
    const size_t n = sc.n;
    int k = 0;
    size_t i = 0;
    while (i < n) {
        const uint8_t op = p[i++];
        size_t len;
        if (op <= 75) {
            len = op;
        } else if (op == 0x4c) {
            if (i >= n) return -1;
            len = p[i++];
        } else if (op == 0x4d) {
            if (i + 2 > n) return -1;
            len = p[i] | ((size_t)p[i + 1] << 8);
            i += 2;
        } else {
            return -1;
        }
        if (i + len > n || k >= cap) return -1;
        out[k].p = p + i;
        out[k].n = len;
        k++;
        i += len;
    }
    return k;
}

bool early_sighash_job(EarlyShard& es, TxEntry& te, unsigned nin, const Span& code, int hashtype,
                       uint32_t row);

// The item's candidate (key, signature) pairs by the shape of its spent script and its input.
// Legacy candidates (P2PKH, P2SH multisig, P2PK) of a long template with SIGHASH_ALL also get an
// early sighash job over the scriptCode the interpreter will use (the spent script, or the redeem
// script), so that the round's longest chains run during the host pass too.
void early_extract_item(Item& it, EarlyShard& es) {
    it.ec_first = (uint32_t)es.cands.size();
    it.ec_count = 0;
    const bcc_batch_item* in = it.in;
    const uint8_t* spk = in->script_pubkey;
    const size_t L = in->script_pubkey_len;
    if (!spk) return;
    const TxIn& txin = it.tx->tx.vin[in->n_in];
    // code.n != 0: a legacy check over that scriptCode (early sighash when the template is long)
    auto add = [&](const Span& pub, const Span& sig, const Span& code = Span{}) {
        uint8_t r[32], s[32];
        if (!tuple_fields(pub.p, pub.n, sig.p, sig.n, r, s)) return;
        const bool k65 = pub.n == 65;
        const uint32_t row = es.rows.add_lazy(pub.p[0], pub.p + 1, r, s, k65 ? pub.p + 33 : nullptr, nullptr);
        if (k65) es.rows.y_unused = false;
        EarlyCand c{pub.p, sig.p, (uint32_t)pub.n, (uint32_t)sig.n, row};
        if (code.n && g_early_sighash && legacy_all_type(sig.p[sig.n - 1]) &&
            early_sighash_job(es, *it.tx, in->n_in, code, sig.p[sig.n - 1], row)) {
            c.code = code.p;
            c.code_len = (uint32_t)code.n;
            c.msg = true;
        }
        es.cands.push_back(c);
        it.ec_count++;
    };
    const auto& wit = txin.witness;
    if (L == 22 && spk[0] == 0x00 && spk[1] == 0x14) {  // P2WPKH: witness [sig, key]
        if (wit.size() == 2) add(wit[1], wit[0]);
        return;
    }
    Span pu[20];
    if (L == 25 && spk[0] == 0x76 && spk[1] == 0xa9 && spk[2] == 0x14 && spk[23] == 0x88 && spk[24] == 0xac) {
        if (script_pushes(txin.script_sig, pu, 2) == 2) add(pu[1], pu[0], Span{spk, L});  // P2PKH
        return;
    }
    if (L == 23 && spk[0] == 0xa9 && spk[1] == 0x14 && spk[22] == 0x87) {  // P2SH
        const int k = script_pushes(txin.script_sig, pu, 20);
        if (k < 1) return;
        const Span& rs = pu[k - 1];
        if (k == 1 && rs.n == 22 && rs.p[0] == 0x00 && rs.p[1] == 0x14) {  // P2SH-P2WPKH
            if (wit.size() == 2) add(wit[1], wit[0]);
            return;
        }
        // m-of-n CHECKMULTISIG redeem script: OP_m <key>... OP_n OP_CHECKMULTISIG, scriptSig
        // OP_0 <sig_1> ... <sig_m> <redeem>: sig i meets keys i .. i + n - m (interpreter.cpp:1176-1205)
        if (rs.n < 3 || rs.p[rs.n - 1] != 0xae) return;
        const int m = rs.p[0] - 0x50, n = rs.p[rs.n - 2] - 0x50;
        if (m < 1 || n < m || n > 16 || k - 2 != m || pu[0].n != 0) return;
        Span keys[16];
        if (script_pushes(Span{rs.p + 1, rs.n - 3}, keys, 16) != n) return;
        if (m * (n - m + 1) > 16) return;
        for (int i = 0; i < m; i++)
            for (int j = i; j <= i + n - m; j++) add(keys[j], pu[1 + i], rs);
        return;
    }
    if (((L == 35 && spk[0] == 33) || (L == 67 && spk[0] == 65)) && spk[L - 1] == 0xac) {  // P2PK
        if (script_pushes(txin.script_sig, pu, 1) == 1) add(Span{spk + 1, L - 2}, pu[0], Span{spk, L});
    }
}

// One round's jobs by kind, added to the calling thread's counts (bcc_last_sighash_kinds).
void count_kinds(const SighashJobs& j, size_t host_hashed) {
    t_kinds.legacy_template += j.tjobs.size();
    t_kinds.legacy_rawtx += j.ljobs.size();
    t_kinds.bip143_rawtx += j.wjobs.size() - j.n_win_single;
    t_kinds.bip143_rawtx_single += j.n_win_single;
    t_kinds.host_preimage += j.pre_off.size();
    t_kinds.single_bug += j.n_single_bug;
    t_kinds.host_hashed += host_hashed;
}

struct Pending {
    uint32_t item;
    uint32_t slot;  // index of the check in the item's cache
};

// Appends the identity of a signature check (sigversion, pubkey, signature, scriptCode) to the
// key arena; returns its length.  A scriptCode longer than 64 bytes enters as its SHA-256 (the
// reference's own signature cache keys entries by a SHA-256 over the check's inputs,
// script/sigcache.cpp ComputeEntryECDSA), so a key costs at most ~1.1 KB however large the
// script: pushes are <= 520 bytes (script.h MAX_SCRIPT_ELEMENT_SIZE).
uint32_t append_key(std::vector<uint8_t>& a, const Bytes& pub, const Bytes& sig, const Bytes& code,
                    SigVersion sv) {
    const size_t k0 = a.size();
    uint8_t d[32];
    const bool hashed = code.size() > 64;
    if (hashed) sha256(code.data(), code.size(), d);
    const uint8_t* cp = hashed ? d : code.data();
    const size_t cn = hashed ? 32 : code.size();
    const size_t len = 1 + 4 + pub.size() + 4 + sig.size() + 1 + 4 + cn;
    a.resize(k0 + len);  // one growth check, then plain stores
    uint8_t* o = &a[k0];
    auto put = [&](const uint8_t* p, size_t n) {
        const uint32_t n32 = (uint32_t)n;
        memcpy(o, &n32, 4);
        if (n) memcpy(o + 4, p, n);
        o += 4 + n;
    };
    *o++ = (uint8_t)sv;
    put(pub.data(), pub.size());
    put(sig.data(), sig.size());
    *o++ = hashed ? 1 : 0;
    put(cp, cn);
    return (uint32_t)len;
}

// The sighash job of one deferred check: what GenericTransactionSignatureChecker would hash
// (SignatureHash, interpreter.cpp:1576-1642) for input in.n_in of te's tx, as a device job whose
// digest lands in tuple row `row` (legacy SIGHASH_ALL: template job; other legacy hashtypes: host
// preimage, SINGLE bug -> the row keeps ONE; BIP143: raw-tx job, SIGHASH_SINGLE: host preimage +
// aux messages).  te's per-round slots (template, aux, raw tx) are filled on first use and te is
// then appended to `touched` (Round::reset clears them).
// BIP143 per-tx chains (hashPrevouts / hashSequence / hashOutputs) of tx, in 64-byte blocks
uint32_t bip143_tx_chain_blocks(const Tx& tx) {
    size_t out = 0;
    for (const TxOut& o : tx.vout) out += o.ser.n;
    return (uint32_t)(sha_padded_len(std::max<size_t>(36 * tx.vin.size(), out)) / 64);
}

// The BIP143 sighash of a long tx's check on the host: the tx's three digests once per round
// (te.hdig), then the check's own preimage.
void host_bip143_sighash(HostJobs& host, TxEntry& te, unsigned nin, const Bytes& code, int hashtype,
                         int64_t amount, std::vector<uint8_t>& scratch, Bip143Job& job,
                         std::vector<TxEntry*>& touched, uint8_t* out32) {
    const Tx& tx = te.tx;
    if (te.hdig < 0) {
        te.hdig = (int32_t)(host.dig.size() / 96);
        host.dig.resize(host.dig.size() + 96);
        for (int k = 0; k < 3; k++) {
            build_aux_message(tx, (AuxKind)k, scratch);
            sha256d(scratch.data(), scratch.size(), &host.dig[96 * (size_t)te.hdig + 32 * k]);
        }
        touched.push_back(&te);
    }
    build_bip143_preimage(tx, nin, code, hashtype, amount, job);
    for (int k = 0; k < 3; k++) {
        if (!job.need[k]) continue;
        if (k == AUX_OUTPUTS && job.single_output) {
            const Span& o = tx.vout[nin].ser;
            sha256d(o.p, o.n, &job.preimage[job.off[k]]);
        } else {
            memcpy(&job.preimage[job.off[k]], &host.dig[96 * (size_t)te.hdig + 32 * k], 32);
        }
    }
    sha256d(job.preimage.data(), job.preimage.size(), out32);
    host.inline_rows++;
}

// `host` (optional): legacy checks whose SHA chain exceeds host->chain_blocks, and every BIP143
// check of a tx whose per-tx chains exceed host->bip143_blocks, are hashed on the host (HostJobs);
// their msg rows in `rows` are materialized (the other rows stay lazy ONE).
// early (round 5): the row's digest also exists in the call's early set; a device template job is
// then flagged TPL_EARLY (the front skips it, the round copies the early digest).  Returns whether
// it was so flagged.
bool add_sighash_job(SighashJobs& jobs, TxEntry& te, const bcc_batch_item& in, const Bytes& code,
                     SigVersion sv, int hashtype, uint32_t row, std::vector<uint8_t>& scratch,
                     Bip143Job& bip143, std::vector<TxEntry*>& touched, HostJobs* host = nullptr,
                     TupleRows* rows = nullptr, bool early = false) {
    bool flagged = false;
    const Tx& tx = te.tx;
    const unsigned nin = in.n_in;
    const uint32_t hb = host && rows ? host->chain_blocks : 0;
    const uint32_t hb143 = host && rows ? host->bip143_blocks : 0;
    auto msg_row = [&]() {
        rows->pad_msg(row + 1);
        return &rows->msg[32 * (size_t)row];
    };
    const bool dev_ht = g_device_hashtypes.load(std::memory_order_relaxed);
    // the tx among the round's raw txs (WtxRec), uploaded on first use
    auto place_wtx = [&](bool table_only) {
        if (te.wtx >= 0) {
            if (!table_only) jobs.wtx[te.wtx].n_in &= ~WTX_TABLE_ONLY;
            return;
        }
        const uint8_t* raw = in.tx_to;
        const size_t len = in.tx_to_len;
        if (tx.has_witness() && !tx.vout.empty() && len > 10) {
            // upload the tx without marker, flag and witnesses (BIP144 layout: the
            // inputs start at byte 6, the outputs end where the witnesses begin)
            const Span& last = tx.vout.back().ser;
            const size_t mid = (size_t)(last.p + last.n - (raw + 6));
            te.wtx = (int32_t)jobs.add_wtx3(raw, 4, raw + 6, mid, raw + len - 4, 4,
                                            tx.vin.size());
            te.wtx_skip = 2;
        } else {
            te.wtx = (int32_t)jobs.add_wtx(raw, len, tx.vin.size());
            te.wtx_skip = 0;
        }
        if (table_only) jobs.wtx[te.wtx].n_in |= WTX_TABLE_ONLY;
        touched.push_back(&te);
    };
    if (sv == SIGVERSION_BASE && legacy_all_type(hashtype)) {
        // device-assembled from the tx template (pipeline.h TplJob), or a host job.  A long
        // template carries its midstates (TPL_MID): a job then hashes only the blocks from its
        // splice on, and the jobs whose remainder exceeds host->chain_blocks (the first inputs of
        // a many-input tx) go to the host while the round's budget lasts.  The template is placed
        // on each side on first use there (host->tpl, jobs.tpl).
        if (te.tpl < 0 && te.htpl < 0) te.tpl_len = (uint32_t)legacy_template_len(tx);
        const bool use_mid = SighashJobs::tpl_nblk(te.tpl_len, 1) >= TPL_MID_MIN_BLOCKS;
        build_script_code_field(code, scratch);
        TplJob tj;
        tj.tpl_len = te.tpl_len;
        tj.pos = (uint32_t)legacy_template_pos(tx, nin);
        tj.code_len = (uint32_t)scratch.size();
        tj.hashtype = (uint32_t)hashtype;
        tj.row = row;
        tj.nblk = SighashJobs::tpl_nblk(tj.tpl_len, tj.code_len) | (use_mid ? TPL_MID : 0u);
        const uint32_t work = tpl_job_blocks(tj);
        const bool on_host = hb && work > hb && host->take(work);
        if ((on_host ? te.htpl : (int64_t)te.tpl) < 0) {
            static thread_local std::vector<uint8_t> tbuf;
            static thread_local std::vector<uint32_t> mbuf;
            build_legacy_template(tx, tbuf);
            const uint32_t* mp = nullptr;
            if (use_mid) {
                tpl_midstates(tbuf.data(), (uint32_t)tbuf.size(), mbuf);
                mp = mbuf.data();
            }
            if (te.tpl < 0 && te.htpl < 0) touched.push_back(&te);
            if (on_host) te.htpl = (int64_t)append_tpl(host->tpl, tbuf.data(), tbuf.size(), mp);
            else te.tpl = jobs.add_tpl(tbuf.data(), tbuf.size(), mp);
        }
        if (on_host) {
            msg_row();  // hash_host_jobs writes the row
            tj.tpl_off = (uint32_t)te.htpl;
            tj.code_off = (uint32_t)host->code.size();
            host->code.insert(host->code.end(), scratch.begin(), scratch.end());
            host->tjobs.push_back(tj);
        } else {
            tj.tpl_off = (uint32_t)te.tpl;
            tj.code_off = jobs.add_code(scratch.data(), scratch.size());
            if (early) tj.nblk |= TPL_EARLY;
            flagged = early;
            jobs.tjobs.push_back(tj);
        }
    } else if (sv == SIGVERSION_BASE && (hashtype & 0x1f) == 3 && nin >= tx.vout.size()) {
        jobs.n_single_bug++;  // SIGHASH_SINGLE bug, msg stays ONE
    } else if (sv == SIGVERSION_BASE && dev_ht) {
        // assembled on the device from the raw tx bytes (pipeline.h LinJob); the lane hashes the
        // whole preimage, so a chain above host->chain_blocks goes to the host as it did
        const bool acp = (hashtype & 0x80) != 0;
        const int base = hashtype & 0x1f;
        build_script_code_field(code, scratch);
        // the output bytes the preimage keeps, as a range of tx_to: the output count follows the
        // last input's nSequence, the outputs end where the last one does
        const uint8_t* oc = tx.vin.back().script_sig.end() + 4;
        const uint8_t *o0 = oc, *o1 = tx.vout.empty() ? oc + 1 : tx.vout.back().ser.end();
        size_t outsec = (size_t)(o1 - o0);
        if (base == 2) {
            o1 = o0;
            outsec = 1;
        } else if (base == 3) {
            o0 = tx.vout[nin].ser.p;
            o1 = tx.vout[nin].ser.end();
            outsec = (nin + 1 < 253 ? 1 : 3) + 9 * (size_t)nin + (size_t)(o1 - o0);
        }
        const size_t nins = acp ? 1 : tx.vin.size();
        const size_t plen = 4 + (nins < 253 ? 1 : nins <= 0xFFFF ? 3 : 5) + 41 * (nins - 1) + 40 +
                            scratch.size() + outsec + 8;
        const uint64_t nb = sha_padded_len(plen) / 64;
        if (hb && nb > hb && host->take(nb)) {
            build_legacy_preimage(tx, nin, code, hashtype, scratch);
            msg_row();
            host->pre.insert(host->pre.end(), scratch.begin(), scratch.end());
            host->pre_off.push_back(host->pre.size());
            host->pre_row.push_back(row);
        } else {
            place_wtx(true);
            LinJob lj{};
            lj.tx = (uint32_t)te.wtx;
            lj.nin = nin;
            lj.code_off = jobs.add_code(scratch.data(), scratch.size());
            lj.code_len = (uint32_t)scratch.size();
            lj.hashtype = (uint32_t)hashtype;
            lj.row = row;
            lj.out_off = (uint32_t)(o0 - in.tx_to) - te.wtx_skip;
            lj.out_len = (uint32_t)(o1 - o0);
            jobs.ljobs.push_back(lj);
        }
    } else if (sv == SIGVERSION_BASE) {
        if (build_legacy_preimage(tx, nin, code, hashtype, scratch)) {
            const uint64_t nb = sha_padded_len(scratch.size()) / 64;
            if (hb && nb > hb && host->take(nb)) {
                msg_row();
                host->pre.insert(host->pre.end(), scratch.begin(), scratch.end());
                host->pre_off.push_back(host->pre.size());
                host->pre_row.push_back(row);
            } else {
                jobs.add_pre(scratch.data(), scratch.size(), row);
            }
        }
    } else if (hb143 && (te.hdig >= 0 ||
                         ((te.wtx < 0 || (jobs.wtx[te.wtx].n_in & WTX_TABLE_ONLY)) &&
                          bip143_tx_chain_blocks(tx) > hb143))) {
        // a long BIP143 tx: every check of it on the host, at once
        host_bip143_sighash(*host, te, nin, code, hashtype, in.amount, scratch, bip143, touched,
                            msg_row());
    } else if ((hashtype & 0x1f) != 3 || dev_ht) {
        // BIP143 assembled on the device from the raw tx bytes (pipeline.h WinJob): the
        // host appends the tx once per round and a record per check
        place_wtx(false);
        WinJob wj{};
        wj.tx = (uint32_t)te.wtx;
        wj.nin = nin;
        wj.code_off = jobs.add_code_field(code.data(), code.size());  // compactsize || code
        wj.code_len = (uint32_t)(code.size() + (code.size() < 253 ? 1 : code.size() <= 0xFFFF ? 3 : 5));
        wj.hashtype = (uint32_t)hashtype;
        wj.row = row;
        wj.amount_lo = (uint32_t)(uint64_t)in.amount;
        wj.amount_hi = (uint32_t)((uint64_t)in.amount >> 32);
        if ((hashtype & 0x1f) == 3) {  // SIGHASH_SINGLE: output nin's range behind the code field
            uint32_t tr[2] = {0, 0};
            if (nin < tx.vout.size()) {
                const Span& o = tx.vout[nin].ser;
                tr[0] = (uint32_t)(o.p - in.tx_to) - te.wtx_skip;
                tr[1] = (uint32_t)o.n;
            }
            const uint8_t* tb = reinterpret_cast<const uint8_t*>(tr);
            jobs.code.insert(jobs.code.end(), tb, tb + 8);
            jobs.n_win_single++;
        }
        jobs.wjobs.push_back(wj);
    } else {  // SIGHASH_SINGLE: host preimage, single-output aux message
        Bip143Job& job = bip143;
        build_bip143_preimage(tx, nin, code, hashtype, in.amount, job);
        uint32_t pre = jobs.add_pre(job.preimage.data(), job.preimage.size(), row);
        size_t base = (size_t)jobs.pre_off[pre] * 64;
        for (int k = 0; k < 3; k++) {
            if (!job.need[k]) continue;
            int32_t aux;
            if (k == AUX_OUTPUTS && job.single_output) {
                const Span& o = tx.vout[nin].ser;
                aux = (int32_t)jobs.add_aux(o.p, o.n);
            } else {
                if (te.aux[k] < 0) {
                    build_aux_message(tx, (AuxKind)k, scratch);
                    te.aux[k] = (int32_t)jobs.add_aux(scratch.data(), scratch.size());
                    touched.push_back(&te);
                }
                aux = te.aux[k];
            }
            jobs.patches.push_back(PatchRec{(uint32_t)(base + job.off[k]), (uint32_t)aux});
        }
    }
    return flagged;
}

// An early sighash job (early Q halves, round 5): the legacy SIGHASH_ALL template job of input
// nin over `code`, as add_sighash_job would build it, with the early row `row` as its output.
// Only long templates (>= TPL_MID_MIN_BLOCKS blocks: the chains that set a small round's front)
// qualify; false = no job.  The template (with midstates) is placed once per tx and shard.
bool early_sighash_job(EarlyShard& es, TxEntry& te, unsigned nin, const Span& code, int hashtype,
                       uint32_t row) {
    const Tx& tx = te.tx;
    if (te.etpl < 0 && te.etpl_len == 0) te.etpl_len = (uint32_t)legacy_template_len(tx);
    if (SighashJobs::tpl_nblk(te.etpl_len, 1) < TPL_MID_MIN_BLOCKS) return false;
    // only the chains that set the round's front: blocks from the splice's midstate on
    const uint32_t pos = (uint32_t)legacy_template_pos(tx, nin);
    const uint32_t cfield = (uint32_t)code.n + (code.n < 253 ? 1 : code.n <= 0xFFFF ? 3 : 5);
    const uint32_t work = SighashJobs::tpl_nblk(te.etpl_len, cfield) - pos / 64;
    const uint32_t hb = g_host_chain_blocks.load(std::memory_order_relaxed);
    if (work < g_early_sighash_min || (hb && work > hb)) return false;  // (longer: the host's)
    SighashJobs& jobs = es.jobs;
    if (te.etpl < 0) {
        static thread_local std::vector<uint8_t> tbuf;
        static thread_local std::vector<uint32_t> mbuf;
        build_legacy_template(tx, tbuf);
        tpl_midstates(tbuf.data(), (uint32_t)tbuf.size(), mbuf);
        te.etpl = jobs.add_tpl(tbuf.data(), tbuf.size(), mbuf.data());
        te.etpl_len = (uint32_t)tbuf.size();
    }
    static thread_local std::vector<uint8_t> field;
    const Bytes c(code.p, code.p + code.n);
    build_script_code_field(c, field);
    TplJob tj;
    tj.tpl_off = (uint32_t)te.etpl;
    tj.tpl_len = te.etpl_len;
    tj.pos = pos;
    tj.code_off = jobs.add_code(field.data(), field.size());
    tj.code_len = (uint32_t)field.size();
    tj.hashtype = (uint32_t)hashtype;
    tj.row = row;
    tj.nblk = SighashJobs::tpl_nblk(tj.tpl_len, tj.code_len) | TPL_MID;
    jobs.tjobs.push_back(tj);
    return true;
}

class Round;

// The deferral seam (BaseSignatureChecker::CheckECDSASignature, interpreter.h:227)
class DeferringChecker : public SigChecker {
public:
    DeferringChecker(Round& rd, uint32_t idx, Item& it) : rd_(rd), idx_(idx), it_(it) {}
    bool check_ecdsa(const Bytes& sig, const Bytes& pub, const Bytes& code, SigVersion sv) override;
    void hint_ecdsa(const Bytes& sig, const Bytes& pub, const Bytes& code, SigVersion sv) override;
    bool hint_all() const override { return it_.runs > 1; }  // a re-run: queue every pair
    const uint8_t* cached_hash160(const uint8_t* p, size_t n) const override {
        return it_.h160_src && n == it_.h160_len && memcmp(p, it_.h160_src, n) == 0 ? it_.h160
                                                                                     : nullptr;
    }
    // first runs only: a re-run (the device found the check or the hash false) compares on the host
    bool defer_key_hash(const uint8_t* key, size_t n, const uint8_t* prog20) override {
        if (it_.runs != 1 || !g_device_key_hash.load(std::memory_order_relaxed) ||
            cached_hash160(key, n))
            return false;
        kh_prog_ = prog20;
        kh_taken_ = false;
        return true;
    }
    bool key_hash_taken() override {
        const bool t = kh_taken_;
        kh_prog_ = nullptr;
        kh_taken_ = false;
        return t;
    }
    bool check_locktime(int64_t n) override { return tx_check_locktime(it_.tx->tx, it_.in->n_in, n); }
    bool check_sequence(int64_t n) override { return tx_check_sequence(it_.tx->tx, it_.in->n_in, n); }

private:
    Round& rd_;
    uint32_t idx_;
    Item& it_;
    const uint8_t* kh_prog_ = nullptr;  // a key-hash condition for the next check_ecdsa
    bool kh_taken_ = false;             // ... which a new device row carries
};

// One GPU round: the tuples deferred by this round's interpreter runs.  One per shard, written by
// its worker: cache-line aligned so that neighbouring shards' Rounds share no line.
class alignas(64) Round {
public:
    SighashJobs jobs;
    TupleRows rows;
    std::vector<Pending> pending;
    std::vector<uint8_t> scratch;
    std::vector<uint8_t> keys;  // check identities of this shard's items (whole call, all rounds)
    Bip143Job bip143;
    std::vector<TxEntry*> touched;
    HostJobs host;  // checks whose sighash the host computes (long chains)
    size_t host_rejected = 0;
    size_t key_hashes = 0;  // key-hash conditions deferred (whole call)
    const EarlyShard* early = nullptr;  // this shard's early rows (whole call; null: none)
    uint32_t erow0 = 0;                 // ... and their first lane in the call's early set
    size_t early_mapped = 0;            // rows mapped to an early twin (whole call)
    size_t early_msgs = 0;              // ... of which take its early sighash (TPL_EARLY)

    // GenericTransactionSignatureChecker::CheckECDSASignature (interpreter.cpp:1656-1676) up to
    // the point where the sighash + secp256k1 verify would run; those become a GPU tuple.
    // consult = false queues a check the run may reach later (a CHECKMULTISIG candidate pair)
    // without making the item's finality depend on it.
    // key_prog (with key_taken): a key-hash condition the new row carries (TupleRows::hrow); a
    // check answered from the item's cache or rejected on the host leaves it to the caller.
    bool defer(uint32_t item_idx, Item& it, const Bytes& sig, const Bytes& pub, const Bytes& code,
               SigVersion sv, bool consult, const uint8_t* key_prog = nullptr,
               bool* key_taken = nullptr) {
        const uint64_t koff = keys.size();
        const uint32_t klen = append_key(keys, pub, sig, code, sv);
        for (const Item::Check& c : it.cache) {
            if (c.len != klen || memcmp(&keys[c.off], &keys[koff], klen) != 0) continue;
            keys.resize(koff);                          // seen before: drop the copy
            if (c.v >= 0) return c.v != 0;              // known
            if (consult) it.pending.push_back((uint32_t)(-2 - c.v));
            return true;                                // deferred this round: speculate
        }
        // an early twin with the same key and signature bytes (early Q halves): its row passed the
        // host filter and holds this check's r and s, and its K_keyq result is reused on the GPU
        const EarlyCand* twin = nullptr;
        if (early) {
            for (uint32_t k = it.ec_first, e = it.ec_first + it.ec_count; k < e; k++) {
                const EarlyCand& c = early->cands[k];
                if (c.publen == pub.size() && c.siglen == sig.size() &&
                    memcmp(c.pub, pub.data(), c.publen) == 0 && memcmp(c.sig, sig.data(), c.siglen) == 0) {
                    twin = &c;
                    break;
                }
            }
        }
        // CPubKey filter, empty signature, lax-DER: decided on the host (no secp work)
        uint8_t r[32], s[32];
        if (twin) {
            memcpy(r, &early->rows.r[32 * (size_t)twin->row], 32);
            memcpy(s, &early->rows.s[32 * (size_t)twin->row], 32);
        } else if (!tuple_fields(pub.data(), pub.size(), sig.data(), sig.size(), r, s)) {
            it.cache.push_back(Item::Check{koff, klen, 0});
            host_rejected++;
            return false;
        }
        const int hashtype = sig.back();
        // y only for a 65-byte key; msg rows stay lazy (uint256 ONE, the SIGHASH_SINGLE-bug
        // message, initialised by the device) unless add_sighash_job hashes the row on the host
        const bool key65 = pub.size() == 65;
        const uint32_t row = rows.add_lazy(pub[0], pub.data() + 1, r, s, key65 ? pub.data() + 33 : nullptr,
                                           nullptr);
        if (key65) rows.y_unused = false;
        if (twin) {
            rows.set_emap(row, erow0 + twin->row);
            early_mapped++;
        }
        if (key_prog) {
            rows.add_key_hash(row, key_prog);
            *key_taken = true;
            key_hashes++;
        }
        // the twin's early sighash is this check's when the interpreter's scriptCode is the one
        // the early job used (legacy, same bytes: FindAndDelete left it alone) -- the hashtype is
        // the signature's last byte, equal by the twin match
        const bool early_msg = twin && twin->msg && sv == SIGVERSION_BASE &&
                               twin->code_len == code.size() &&
                               memcmp(twin->code, code.data(), code.size()) == 0;
        if (add_sighash_job(jobs, *it.tx, *it.in, code, sv, hashtype, row, scratch, bip143, touched,
                            &host, &rows, early_msg)) {
            rows.set_mmap(row, erow0 + twin->row);
            early_msgs++;
        }
        it.cache.push_back(Item::Check{koff, klen, -2 - (int32_t)pending.size()});
        if (consult) it.pending.push_back((uint32_t)pending.size());
        pending.push_back(Pending{item_idx, (uint32_t)(it.cache.size() - 1)});
        return true;  // speculative
    }

    // legacy_host: legacy chains may go to the host (chunk_interpret: every round, one or more GPUs)
    void reset(bool legacy_host = true) {
        jobs.clear();
        rows.clear();
        rows.msg_one = true;   // every row enters with msg = ONE (defer)
        rows.y_unused = true;  // until a 65-byte key is deferred
        pending.clear();
        host.clear();
        host.chain_blocks = legacy_host ? g_host_chain_blocks.load(std::memory_order_relaxed) : 0;
        host.bip143_blocks = g_host_bip143_blocks.load(std::memory_order_relaxed);
        for (auto* t : touched) {
            t->aux[0] = t->aux[1] = t->aux[2] = -1;
            t->tpl = -1;
            t->wtx = -1;
            t->htpl = -1;
            t->hdig = -1;
        }
        touched.clear();
    }
};

// Marks the rows of every shard with host-written messages for upload (inline BIP143 rows now,
// offloaded jobs' rows before or during the device round).  Returns whether any job is pending.
bool mark_host_rows(std::vector<Round>& rds, unsigned T) {
    bool any = false;
    for (unsigned t = 0; t < T; t++) {
        HostJobs& h = rds[t].host;
        if (h.pending() || h.inline_rows) {
            rds[t].rows.msg_one = false;
            rds[t].rows.pad_msg(rds[t].rows.size());
        }
        any |= h.pending() != 0;
    }
    return any;
}

// The offloaded legacy jobs of the shards `shards`, hashed in parallel on the calling thread's team
// (their rows' msg receive the sighash).
void hash_host_jobs(std::vector<Round>& rds, const std::vector<unsigned>& shards, unsigned maxW = 0) {
    std::vector<std::pair<uint32_t, uint32_t>> work;  // (shard, job): tjobs first, then pre
    for (unsigned t : shards)
        for (uint32_t k = 0; k < rds[t].host.pending(); k++) work.emplace_back(t, k);
    if (work.empty()) return;
    size_t blocks = 0;
    for (const auto& w : work) {
        const HostJobs& h = rds[w.first].host;
        blocks += w.second < h.tjobs.size() ? tpl_job_blocks(h.tjobs[w.second]) : 8;
    }
    const unsigned T = (unsigned)shards.size();
    const unsigned W = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(maxW ? maxW : T, host_threads()),
                                                                         blocks / 256 + 1));
    // jobs are dealt round-robin: the long ones of one tx are spread over every worker
    run_team(W, [&](unsigned w) {
        for (size_t i = w; i < work.size(); i += W) {
            Round& rd = rds[work[i].first];
            HostJobs& h = rd.host;
            uint8_t* out = rd.rows.msg.data();
            const uint32_t k = work[i].second;
            if (k < h.tjobs.size()) {
                const TplJob& t = h.tjobs[k];
                tpl_job_sighash(h.tpl.data(), h.code.data(), t, out + 32 * (size_t)t.row);
            } else {
                const size_t j = k - h.tjobs.size();
                sha256d(&h.pre[h.pre_off[j]], h.pre_off[j + 1] - h.pre_off[j],
                        out + 32 * (size_t)h.pre_row[j]);
            }
        }
    });
}

void hash_host_jobs(std::vector<Round>& rds, unsigned T, unsigned maxW = 0) {
    std::vector<unsigned> all(T);
    for (unsigned t = 0; t < T; t++) all[t] = t;
    hash_host_jobs(rds, all, maxW);
}

// A round's offloaded jobs hashed while the device runs: the device round calls ensure() through
// its LateMsgFill once the message-independent kernels are queued; every host path that needs the
// messages calls it first.  Hashes each shard once per interpreter pass.
// Multi-GPU rounds (round 6, after the round-5 advisory): each device group's fill hashes only its
// own shards [g0, g1) -- concurrently with the other groups, on its worker's team -- so no worker
// ever writes the msg rows of a shard another worker is staging (copy_msg).  A shard another
// caller has claimed is waited for, never hashed twice.  The hashing time is kept here for the
// caller's statistics (chunk_finish), not added to the calling thread's t_stats: on a pipeline or
// device worker that would have been the worker's.
struct LateHost {
    std::vector<Round>* rds = nullptr;
    unsigned T = 0;
    unsigned W = 0;       // worker threads (0: at most the shards hashed)
    double seconds = 0;   // hashing time, collected by chunk_finish (read with no round running)
    struct Sync {
        std::mutex mu;
        std::condition_variable cv;
        std::vector<uint8_t> state;  // per shard: 0 to hash, 1 being hashed, 2 done
    };
    std::shared_ptr<Sync> sy = std::make_shared<Sync>();
    LateHost() = default;
    LateHost(std::vector<Round>* r, unsigned t, unsigned w) : rds(r), T(t), W(w) {}
    void ensure() { ensure(0, T); }
    void ensure(unsigned lo, unsigned hi) {
        std::vector<unsigned> mine;
        {
            std::lock_guard<std::mutex> lk(sy->mu);
            if (sy->state.size() != T) sy->state.assign(T, 0);
            for (unsigned t = lo; t < hi; t++)
                if (sy->state[t] == 0) {
                    sy->state[t] = 1;
                    mine.push_back(t);
                }
        }
        if (!mine.empty()) {
            auto h0 = std::chrono::steady_clock::now();
            hash_host_jobs(*rds, mine, W);
            const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - h0).count();
            std::lock_guard<std::mutex> lk(sy->mu);
            for (unsigned t : mine) sy->state[t] = 2;
            seconds += dt;
            sy->cv.notify_all();
        }
        std::unique_lock<std::mutex> lk(sy->mu);
        sy->cv.wait(lk, [&] {
            for (unsigned t = lo; t < hi; t++)
                if (sy->state[t] != 2) return false;
            return true;
        });
    }
};

bool DeferringChecker::check_ecdsa(const Bytes& sig, const Bytes& pub, const Bytes& code,
                                   SigVersion sv) {
    const uint8_t* kp = kh_prog_;
    kh_prog_ = nullptr;
    return rd_.defer(idx_, it_, sig, pub, code, sv, true, kp, &kh_taken_);
}

void DeferringChecker::hint_ecdsa(const Bytes& sig, const Bytes& pub, const Bytes& code,
                                  SigVersion sv) {
    rd_.defer(idx_, it_, sig, pub, code, sv, false);
}

int set_err(bitcoinconsensus_error* e, bitcoinconsensus_error v) {
    if (e) *e = v;
    return 0;
}

struct BatchState {
    std::vector<Item> st;
    // one entry per run of adjacent items with the same tx buffer (the inputs of one tx are
    // passed together): each tx is deserialized once and its BIP143 hashes computed once; a
    // buffer repeated non-adjacently is merely parsed again (same result)
    std::vector<TxEntry> txs;
    std::vector<uint32_t> tx_first;  // first item of each entry
    std::vector<std::vector<uint32_t>> tx_slices;  // per-thread scans building tx_first
    unsigned flags = 0;
    size_t n = 0;  // items of the current call: st / txs only grow (a shrink would free every
                   // dropped Item's / TxEntry's buffers, and the next larger call re-allocate them)
};

// Runs f(t) for t in [0, T) on the calling thread's persistent team (inline when T == 1).
template <class F>
void run_threads(unsigned T, F f) {
    run_team(T, std::function<void(unsigned)>(f));
}

// Runs f(s) for every shard s in [0, S) on W of the calling thread's team workers: with S == W one
// shard per worker, with more shards than workers each worker takes the next unstarted shard, so a
// slow shard no longer sets the pass's length (round 5: C3's interpreter shards ran 1.3-1.5x the
// mean on the slowest one at 16 shards).
template <class F>
void run_shards(unsigned S, unsigned W, F f) {
    if (W >= S) {
        run_threads(S, f);
        return;
    }
    std::atomic<unsigned> next{0};
    run_threads(W, [&](unsigned) {
        for (unsigned s; (s = next.fetch_add(1, std::memory_order_relaxed)) < S;) f(s);
    });
}

// Contiguous [lo, hi) share t of T over n units.
inline size_t share_lo(size_t n, unsigned t, unsigned T) { return n * t / T; }

// Boundaries of T contiguous shards of whole tx entries (items of one entry share its TxEntry,
// whose BIP143 aux slots and legacy template the shard's Round owns; prepare cuts a many-input tx
// into several entries), balanced by count: shard t is items [bound[t], bound[t + 1]).
std::vector<size_t> shard_bounds(const BatchState& b, unsigned T) {
    const size_t n = b.n, E = b.tx_first.size();
    std::vector<size_t> bound(T + 1, n);
    bound[0] = 0;
    for (unsigned t = 0; t + 1 < T; t++) {  // the first tx starting at or after the even split
        const size_t want = share_lo(n, t + 1, T);
        auto it = std::lower_bound(b.tx_first.begin(), b.tx_first.end(), (uint32_t)want);
        bound[t + 1] = std::max(bound[t], it == b.tx_first.end() ? n : (size_t)*it);
    }
    (void)E;
    return bound;
}

// verify_script's pre-checks (bitcoinconsensus.cpp:83-95) in reference order.  Tx buffers are
// deserialized once per adjacent run of items, in parallel over T threads.
// With `shards` / `runs`, the workers' shares are the shard_bounds() shards, and each worker also
// fills its shard's item list and run list (the items that passed the pre-checks).
// fused (optional, with `runs`): the first interpreter pass runs inside the parse pass, shard t's
// newly active items handed over every FUSE_BLOCK items while their tx bytes and entries are still
// in cache (chunk_start; not with `early`, which needs every shard parsed first).
using FusedPass = std::function<void(unsigned, const uint32_t*, size_t)>;
constexpr size_t FUSE_BLOCK = 256;
void prepare(BatchState& b, const bcc_batch_item* items, size_t n, unsigned flags, unsigned T,
             std::vector<std::vector<uint32_t>>* shards = nullptr,
             std::vector<std::vector<uint32_t>>* runs = nullptr,
             std::vector<EarlyShard>* early = nullptr, unsigned W = 0,
             const FusedPass* fused = nullptr,
             const std::function<void(unsigned)>* shard_done = nullptr) {
    if (W == 0 || W > T) W = T;  // worker threads over the T shards (run_shards)
    if (b.st.size() < n) b.st.resize(n);  // reused across calls: every field is (re)set below
    b.n = n;
    b.flags = flags;
    auto& st = b.st;
    const bool flags_ok = (flags & ~(unsigned)FLAGS_VERIFY_ALL) == 0;
    // runs of adjacent items with the same tx buffer: scanned in T slices, then concatenated
    auto starts_tx = [&](size_t i) {
        return i == 0 || items[i].tx_to != items[i - 1].tx_to || items[i].tx_to_len != items[i - 1].tx_to_len;
    };
    b.tx_first.clear();
    // A run longer than a quarter of a shard (a many-input tx) is cut into pieces of at most that
    // many items, each its own TxEntry (the tx parsed once per piece, with its own per-round
    // template / aux slots), so that shard_bounds can balance the interpreter passes: C3's
    // 442-input txs made one shard 2.4x the mean (bcc_batch_stats interpret_shard_*).
    const size_t M = std::max<size_t>(32, n / (4 * (size_t)std::max(1u, T)));
    bool longrun = false;
    if (T <= 1 || n < 1024) {
        for (size_t i = 0; i < n; i++)
            if (starts_tx(i)) b.tx_first.push_back((uint32_t)i);
        for (size_t k = 0; T > 1 && k < b.tx_first.size() && !longrun; k++)
            longrun = (k + 1 < b.tx_first.size() ? b.tx_first[k + 1] : n) - b.tx_first[k] > M;
    } else {
        b.tx_slices.resize(T);
        std::vector<size_t> gap(T, 0);  // per slice: the longest run between its own starts
        run_shards(T, W, [&](unsigned t) {
            // appended through a local header (swapped in and out): the shards' vector headers
            // share cache lines, and a push_back per item on them cost every writer its line
            // (round 5: prepare's per-item time 10x single-threaded at 8-16 threads)
            std::vector<uint32_t> v;
            v.swap(b.tx_slices[t]);
            v.clear();
            size_t g = 0;
            for (size_t i = share_lo(n, t, T); i < share_lo(n, t + 1, T); i++)
                if (starts_tx(i)) {
                    if (!v.empty()) g = std::max<size_t>(g, i - v.back());
                    v.push_back((uint32_t)i);
                }
            gap[t] = g;
            v.swap(b.tx_slices[t]);
        });
        size_t total = 0;
        for (unsigned t = 0; t < T; t++) total += b.tx_slices[t].size();
        b.tx_first.resize(total);
        size_t at = 0;
        for (unsigned t = 0; t < T; t++) {
            std::copy(b.tx_slices[t].begin(), b.tx_slices[t].end(), b.tx_first.begin() + at);
            at += b.tx_slices[t].size();
        }
        // the runs inside each slice, then the ones across slice boundaries (a slice's last start
        // to the next start of any later slice, or n)
        size_t next = n;
        for (unsigned t = T; t-- > 0 && !longrun;) {
            const auto& v = b.tx_slices[t];
            if (v.empty()) continue;
            longrun = gap[t] > M || next - v.back() > M;
            next = v.front();
        }
    }
    if (T > 1) {
        if (longrun) {
            std::vector<uint32_t> cut;
            cut.reserve(b.tx_first.size() + n / M + 1);
            for (size_t k = 0; k < b.tx_first.size(); k++) {
                const size_t end = k + 1 < b.tx_first.size() ? b.tx_first[k + 1] : n;
                for (size_t i = b.tx_first[k]; i < end; i += M) cut.push_back((uint32_t)i);
            }
            b.tx_first.swap(cut);
        }
    }
    const size_t E = b.tx_first.size();
    if (b.txs.size() < E) b.txs.resize(E);  // grow only, like st
    // per-thread timing (bcc_batch_stats prepare_*): dispatch -> start lag, parse, batched HASH160
    using pclk = std::chrono::steady_clock;
    std::vector<double> lag(T, 0), tparse(T, 0), thash(T, 0);
    const auto d0 = pclk::now();
    const std::vector<size_t> bound = shard_bounds(b, T);
    if (shards) {
        shards->resize(T);
        runs->resize(T);
    }
    run_shards(T, W, [&](unsigned t) {
        const auto s0 = pclk::now();
        lag[t] = std::chrono::duration<double>(s0 - d0).count();
        // this worker's txs: the entries starting in its shard [bound[t], bound[t + 1])
        const size_t klo = (size_t)(std::lower_bound(b.tx_first.begin(), b.tx_first.end(),
                                                     (uint32_t)bound[t]) - b.tx_first.begin());
        const size_t khi = (size_t)(std::lower_bound(b.tx_first.begin(), b.tx_first.end(),
                                                     (uint32_t)bound[t + 1]) - b.tx_first.begin());
        // the shard / run lists through local headers (see tx_slices above)
        std::vector<uint32_t> lsh, lrl;
        std::vector<uint32_t>* sh = shards ? &lsh : nullptr;
        std::vector<uint32_t>* rl = shards ? &lrl : nullptr;
        if (sh) {
            lsh.swap((*shards)[t]);
            lrl.swap((*runs)[t]);
            sh->clear();
            rl->clear();
        }
        size_t fused_done = 0;  // run-list items already handed to the fused pass
        for (size_t k = klo; k < khi; k++) {
            const bcc_batch_item* in = &items[b.tx_first[k]];
            TxEntry& e = b.txs[k];
            e.aux[0] = e.aux[1] = e.aux[2] = -1;  // every per-round slot (Round::reset's set)
            e.tpl = -1;
            e.wtx = -1;
            e.htpl = -1;
            e.hdig = -1;
            e.etpl = -1;
            e.etpl_len = 0;
            e.ok = flags_ok && in->tx_to != nullptr && parse_tx(in->tx_to, in->tx_to_len, e.tx);
            const size_t end = k + 1 < E ? b.tx_first[k + 1] : n;
            for (size_t i = b.tx_first[k]; i < end; i++) {
                Item& it = st[i];
                it.in = &items[i];
                it.tx = &e;
                it.ret = 0;
                it.active = false;
                it.result = false;
                it.runs = 0;
                it.cache.clear();
                it.pending.clear();
                it.ec_first = it.ec_count = 0;
                if (!flags_ok) it.err = bitcoinconsensus_ERR_INVALID_FLAGS;
                else if (!e.ok) it.err = bitcoinconsensus_ERR_TX_DESERIALIZE;
                else if (items[i].n_in >= e.tx.vin.size()) it.err = bitcoinconsensus_ERR_TX_INDEX;
                else if (e.tx.ser_size != items[i].tx_to_len) it.err = bitcoinconsensus_ERR_TX_SIZE_MISMATCH;
                else {
                    it.err = bitcoinconsensus_ERR_OK;
                    it.active = true;
                }
                if (sh) {
                    sh->push_back((uint32_t)i);
                    if (it.active) rl->push_back((uint32_t)i);
                }
            }
            if (fused && rl && (rl->size() - fused_done >= FUSE_BLOCK || k + 1 == khi)) {
                (*fused)(t, rl->data() + fused_done, rl->size() - fused_done);
                fused_done = rl->size();
            }
        }
        if (sh) {
            lsh.swap((*shards)[t]);
            lrl.swap((*runs)[t]);
        }
        if (shard_done) (*shard_done)(t);  // (with the fused pass: shard t's rows are final)
        if (early) {  // early Q halves: this shard's candidates while its txs are in cache
            EarlyShard& es = (*early)[t];
            es.clear();
            for (size_t i = bound[t]; i < bound[t + 1]; i++)
                if (st[i].active) early_extract_item(st[i], es);
        }
        const auto s1 = pclk::now();
        tparse[t] = std::chrono::duration<double>(s1 - s0).count();
        // HASH160 of every P2WPKH witness key of this thread's share, eight at a time (the
        // interpreter's OP_HASH160 finds it by content, DeferringChecker::cached_hash160)
        const size_t i0 = bound[t], i1 = bound[t + 1];
        const bool hash_here = !g_device_key_hash.load(std::memory_order_relaxed);
        constexpr size_t BATCH = 64;
        const uint8_t* hp[BATCH];
        size_t hn[BATCH];
        uint8_t* ho[BATCH];
        size_t k = 0;
        auto flush = [&] {
            if (k) hash160_batch(hp, hn, ho, k);
            k = 0;
        };
        for (size_t i = i0; i < i1; i++) {
            Item& it = st[i];
            it.h160_src = nullptr;
            if (!it.active || !hash_here) continue;
            const bcc_batch_item* in = it.in;
            const uint8_t* spk = in->script_pubkey;
            if (in->script_pubkey_len != 22 || spk[0] != 0x00 || spk[1] != 0x14) continue;
            const auto& wit = it.tx->tx.vin[in->n_in].witness;
            if (wit.size() != 2 || (wit[1].n != 33 && wit[1].n != 65)) continue;
            it.h160_src = wit[1].p;
            it.h160_len = (uint32_t)wit[1].n;
            hp[k] = wit[1].p;
            hn[k] = wit[1].n;
            ho[k] = it.h160;
            if (++k == BATCH) flush();
        }
        flush();
        thash[t] = std::chrono::duration<double>(pclk::now() - s1).count();
    });
    for (unsigned t = 0; t < T; t++) {
        t_stats.prepare_lag_seconds = std::max(t_stats.prepare_lag_seconds, lag[t]);
        t_stats.prepare_parse_seconds = std::max(t_stats.prepare_parse_seconds, tparse[t]);
        t_stats.prepare_hash_seconds = std::max(t_stats.prepare_hash_seconds, thash[t]);
    }
}

// Interpreter pass over the active items of one shard (idx: the shard's items that need a run);
// deferred checks land in rd.  Returns whether any item ran.
bool interpret_items(BatchState& b, const uint32_t* idx, size_t m, Round& rd) {
    bool any = false;
    for (size_t k = 0; k < m; k++) {
        const uint32_t i = idx[k];
        Item& it = b.st[i];
        if (!it.active) continue;
        any = true;
        it.runs++;
        it.pending.clear();
        DeferringChecker chk(rd, i, it);
        const TxIn& in = it.tx->tx.vin[it.in->n_in];
        Span spk{it.in->script_pubkey, it.in->script_pubkey_len};
        ScriptErr se;
        try {
            it.result = verify_script(in.script_sig, spk, in.witness, b.flags, chk, &se);
        } catch (...) {  // bitcoinconsensus.cpp:99: any std::exception -> TX_DESERIALIZE
            it.result = false;
            it.err = bitcoinconsensus_ERR_TX_DESERIALIZE;
            it.pending.clear();
        }
        it.active = false;
    }
    return any;
}

bool interpret_shard(BatchState& b, const std::vector<uint32_t>& idx, Round& rd) {
    return interpret_items(b, idx.data(), idx.size(), rd);
}

// One device round over the parts [p0, p1): fault injection first, then the device pipeline.
// A pending injected fault (bcc_debug_fail_device_rounds): its code, consumed; else 0.
int take_injected_fault() {
    for (int f = g_fail_rounds.load(); f > 0;)
        if (g_fail_rounds.compare_exchange_weak(f, f - 1)) return g_fail_code.load();
    return 0;
}

int device_round(int dev, const SighashJobs* const* pj, const TupleRows* const* pr, size_t P,
                 uint8_t* verdict, double* stage_s, const LateMsgFill* late) {
    if (int e = take_injected_fault()) return e;
    return gpu_verify_parts(dev, pj, pr, P, verdict, stage_s, late);
}

}  // namespace

int injected_device_fault() { return take_injected_fault(); }
bool retryable_device_error(int hip_error) { return retryable(hip_error); }

int resilient_round(int dev, const SighashJobs* const* pj, const TupleRows* const* pr, size_t P,
                    uint8_t* verdict, double* stage_s, size_t* retries, size_t* host_rounds,
                    const char* who, const LateMsgFill* late) {
    int e = device_round(dev, pj, pr, P, verdict, stage_s, late);
    if (e != 0 && retryable(e)) {
        fprintf(stderr, "[bcc] %s: device %d round failed (hip error %d), retrying\n", who, dev, e);
        (*retries)++;
        e = device_round(dev, pj, pr, P, verdict, stage_s, late);
    }
    if (e == 0) return 0;
    if (!host_fallback_enabled()) {
        fprintf(stderr, "[bcc] %s: device %d round failed (hip error %d), no verdict "
                        "(BCC_DEVICE_FAILURE_ERROR)\n", who, dev, e);
        return e;
    }
    size_t n = 0;
    for (size_t p = 0; p < P; p++) n += pr[p]->size();
    fprintf(stderr, "[bcc] %s: device %d round failed (hip error %d): verifying its %zu checks on "
                    "the host CPU\n", who, dev, e, n);
    if (late) {  // the late rows' messages into the host rows
        std::vector<uint32_t> lr;
        std::vector<uint8_t> ld;
        (*late)(lr, ld);
    }
    host_verify_parts(pj, pr, P, verdict, host_threads());
    note_host_fallback();
    (*host_rounds)++;
    return 0;
}

namespace {

// Shards [t0, t1) of the round on device `dev`, as device batches whose blobs stay under
// ROUND_BLOB_LIMIT (the device job records use 32-bit byte offsets): consecutive shards are
// grouped greedily; a single shard above the limit is an error (reported, never silently
// truncated).  A batch failing with a transient error is retried once on a fresh device batch
// (gpu_verify_parts drops the failed one); *retries counts those.  If the device still cannot
// deliver, the failure policy decides: the batch is verified on the host (*host_rounds counts
// those) or the error is returned.  Returns 0 or the error.
// The late rows of shards [g0, g1) of `rds` (batch-local), after the host jobs are hashed.
void late_rows(const std::vector<Round>& rds, const std::vector<size_t>& row0, unsigned g0,
               unsigned g1, std::vector<uint32_t>& rows, std::vector<uint8_t>& digs) {
    for (unsigned t = g0; t < g1; t++) {
        const Round& rd = rds[t];
        const uint32_t base = (uint32_t)(row0[t] - row0[g0]);
        auto put = [&](uint32_t r) {
            rows.push_back(base + r);
            const uint8_t* m = &rd.rows.msg[32 * (size_t)r];
            digs.insert(digs.end(), m, m + 32);
        };
        for (const TplJob& tj : rd.host.tjobs) put(tj.row);
        for (uint32_t r : rd.host.pre_row) put(r);
    }
}

// `late` (optional): the group's offloaded host jobs are hashed during each device batch and their
// rows' messages delivered through LateMsgFill.
int run_device_group(int dev, const std::vector<Round>& rds, unsigned t0, unsigned t1,
                     const std::vector<size_t>& row0, uint8_t* verdict, double* stage_total,
                     size_t* retries, size_t* host_rounds, LateHost* late) {
    unsigned g0 = t0;
    while (g0 < t1) {
        size_t sz[5] = {0, 0, 0, 0, 0};
        unsigned g1 = g0;
        for (; g1 < t1; g1++) {
            const SighashJobs& j = rds[g1].jobs;
            const size_t add[5] = {j.aux.size(), j.pre.size(), j.tpl.size(), j.code.size(),
                                   j.txraw.size()};
            bool fits = true;
            for (int k = 0; k < 5; k++) fits &= sz[k] + add[k] <= ROUND_BLOB_LIMIT;
            if (!fits) break;
            for (int k = 0; k < 5; k++) sz[k] += add[k];
        }
        const bool too_big = g1 == g0;
        if (too_big) {
            fprintf(stderr, "[bcc] verify_batch: one shard's sighash jobs exceed %zu bytes\n",
                    ROUND_BLOB_LIMIT);
            g1 = g0 + 1;
        }
        std::vector<const SighashJobs*> pj;
        std::vector<const TupleRows*> pr;
        for (unsigned t = g0; t < g1; t++) {
            pj.push_back(&rds[t].jobs);
            pr.push_back(&rds[t].rows);
        }
        // the late rows of shards [g0, g1), batch-local
        const LateMsgFill fill = [&, g0, g1](std::vector<uint32_t>& rows, std::vector<uint8_t>& digs) {
            late->ensure(g0, g1);  // this group's shards only (the other workers stage theirs)
            late_rows(rds, row0, g0, g1, rows, digs);
        };
        double st = 0;
        int e = 1;
        if (too_big) {
            if (late) late->ensure(g0, g1);
            if (host_fallback_enabled()) {
                host_verify_parts(pj.data(), pr.data(), pj.size(), verdict + row0[g0], host_threads());
                note_host_fallback();
                (*host_rounds)++;
                e = 0;
            }
        } else {
            e = resilient_round(dev, pj.data(), pr.data(), pj.size(), verdict + row0[g0], &st,
                                retries, host_rounds, "verify_batch", late ? &fill : nullptr);
        }
        if (e != 0) return e;
        *stage_total += st;
        g0 = g1;
    }
    return 0;
}

// One device round of the batch: the shards' deferred checks are cut into contiguous groups of
// whole shards with about equal tuple counts, one per configured GPU (shard by
// transaction, so each tx's BIP143 aux hashes stay on one device); the groups run concurrently on
// the GPUs' worker threads and write their verdicts at their row offsets.
int run_device_round(const std::vector<Round>& rds, unsigned T, const std::vector<size_t>& row0,
                     uint8_t* verdict, double* stage_total, size_t* devices_used,
                     size_t* retries, size_t* host_rounds, LateHost* late) {
    if (row0[T] <= host_small_round()) {  // a small round: lower latency on the host CPU
        if (late) late->ensure();
        std::vector<const SighashJobs*> pj;
        std::vector<const TupleRows*> pr;
        for (unsigned t = 0; t < T; t++) {
            pj.push_back(&rds[t].jobs);
            pr.push_back(&rds[t].rows);
        }
        (*host_rounds)++;
        return host_verify_parts(pj.data(), pr.data(), T, verdict, host_threads());
    }
    const std::vector<int> devs = device_list();
    std::vector<size_t> w(T);
    for (unsigned t = 0; t < T; t++) w[t] = rds[t].pending.size();
    const size_t D = std::min<size_t>(devs.size(), T);
    const std::vector<size_t> cut = split_balanced(w, D);
    std::vector<double> st(D, 0);
    std::vector<size_t> rt(D, 0), hr(D, 0);
    std::vector<std::function<int()>> jobs;
    std::vector<int> jd;
    for (size_t d = 0; d < D; d++) {
        if (cut[d] == cut[d + 1]) continue;
        jd.push_back(devs[d]);
        jobs.push_back([&, d] {
            return run_device_group(devs[d], rds, (unsigned)cut[d], (unsigned)cut[d + 1], row0,
                                    verdict, &st[d], &rt[d], &hr[d], late);
        });
    }
    const int e = jobs.empty() ? 0 : run_on_devices(jd, jobs);
    for (size_t d = 0; d < D; d++) {
        *stage_total += st[d];
        *retries += rt[d];
        *host_rounds += hr[d];
    }
    *devices_used = std::max(*devices_used, jobs.size());
    return e;
}

// One chunk of a batch: its host state, its rounds and its device round in flight.  Chunks of one
// call are independent (every item's verdict depends on its own tx only).
struct ChunkRun {
    BatchState b;
    std::vector<Round> rds;
    std::vector<std::vector<uint32_t>> shards, run_list, next_list;
    std::vector<size_t> row0;
    std::vector<uint8_t> verdict;
    unsigned T = 1;  // shards (one Round each)
    unsigned W = 1;  // worker threads over the shards (run_shards)
    size_t n = 0, npend = 0;
    bool pending_round = false;  // a device round for the current run lists is due
    std::future<int> fut;        // the device round in flight (pipelined)
    int sync_rc = 0;             // result of a synchronous device round
    double stage_s = 0;
    size_t devices_used = 0, retries = 0, host_rounds = 0;
    // the first device round of a pipelined chunk, staged by the caller (prestage_round)
    std::unique_ptr<StagedRound, void (*)(StagedRound*)> staged{nullptr, gpu_staged_free};
    bool prestaged = false;
    bool launched = false;  // the prestaged round is already queued on the GPU (chunk_launch)
    std::vector<EarlyShard> early;  // per shard: pre-extracted rows (early Q halves)
    LateHost late;               // offloaded host jobs of the current pass (hashed during the round)
    // their blocks (HostJobs::take); held by pointer so that ChunkRun stays movable
    std::unique_ptr<std::atomic<uint64_t>> host_planned = std::make_unique<std::atomic<uint64_t>>(0);
    bool late_pending = false;
    bool pipelined = false;  // a chunk of a pipelined call (its round goes to `staged`)
};

// Host state of bitcoinconsensus_verify_batch, per calling thread, reused across its calls: two
// chunk slots (one on the host, one on the device when pipelined).
thread_local ChunkRun tl_chunk[2];

using clk = std::chrono::steady_clock;
inline double since(clk::time_point a) { return std::chrono::duration<double>(clk::now() - a).count(); }

// CPU time of every thread of the process so far (bcc_batch_stats process_cpu_*)
inline double process_cpu() {
    timespec ts;
    return clock_gettime(CLOCK_PROCESS_CPUTIME_ID, &ts) == 0 ? ts.tv_sec + 1e-9 * ts.tv_nsec : 0.0;
}

// One interpreter pass over the chunk's run lists; sets up the device round it needs (if any).
void chunk_interpret_finish(ChunkRun& c, const std::vector<char>& ran, const std::vector<double>& ts);

void chunk_interpret(ChunkRun& c) {
    std::vector<char> ran(c.T, 0);
    auto i0 = clk::now();
    c.host_planned->store(0, std::memory_order_relaxed);
    std::vector<double> ts(c.T, 0);
    run_shards(c.T, c.W, [&](unsigned t) {
        auto s0 = clk::now();
        c.rds[t].reset(true);
        c.rds[t].host.planned = c.host_planned.get();
        ran[t] = interpret_shard(c.b, c.run_list[t], c.rds[t]);
        ts[t] = since(s0);
    });
    t_stats.interpret_seconds += since(i0);
    chunk_interpret_finish(c, ran, ts);
}

// What follows an interpreter pass: its statistics, the late host jobs, the round's row offsets.
void chunk_interpret_finish(ChunkRun& c, const std::vector<char>& ran, const std::vector<double>& ts) {
    double tmax = 0, tsum = 0;
    for (double x : ts) {
        tmax = std::max(tmax, x);
        tsum += x;
    }
    t_stats.interpret_shard_max_seconds += tmax;
    t_stats.interpret_shard_mean_seconds += tsum / c.T;
    // the offloaded jobs' rows are marked now; the host hashes the jobs while the device(s) run the
    // message-independent kernels (LateHost; every device worker's round waits for them)
    t_stats.host_jobs_seconds += c.late.seconds;  // a previous pass's hashing (pipelined chunks)
    c.late = LateHost(&c.rds, c.T, c.W);
    c.late_pending = mark_host_rows(c.rds, c.T);
    size_t npend = 0;
    bool any = false;
    for (unsigned t = 0; t < c.T; t++) {
        c.row0[t] = npend;
        npend += c.rds[t].pending.size();
        any |= ran[t] != 0;
    }
    c.row0[c.T] = npend;
    c.npend = npend;
    c.pending_round = any && npend != 0;
    if (!c.pending_round) return;
    for (unsigned t = 0; t < c.T; t++) {
        t_stats.preimages += c.rds[t].jobs.pre_off.size() + c.rds[t].jobs.tjobs.size() +
                             c.rds[t].jobs.wjobs.size();
        t_stats.aux_messages += c.rds[t].jobs.aux_off.size() + 3 * c.rds[t].jobs.wtx.size();
        t_stats.host_hashed += c.rds[t].host.pending() + c.rds[t].host.inline_rows;
        count_kinds(c.rds[t].jobs, c.rds[t].host.pending() + c.rds[t].host.inline_rows);
    }
    t_stats.rounds++;
    t_stats.tuples += npend;
    c.verdict.assign(npend, 0);
}

constexpr size_t SHORT_PASS_ITEMS = 65536;
// Shards per worker of a short pass (BCC_SHARDS_PER_WORKER, default 1).  Round 5 measured 2 and 4
// (dynamically dealt, run_shards) on C3: slower (4.0-4.4 vs 4.7-5.0 M inputs/s,
// profiles/r05/c3/shards): a many-input tx is cut into more pieces, each parsing the tx and
// building its template (and midstates) again, which costs more than the balance gains.
unsigned SHARDS_PER_WORKER = [] {
    const char* e = getenv("BCC_SHARDS_PER_WORKER");
    return e ? std::max(1, atoi(e)) : 1;
}();

// The first interpreter pass fused into the parse pass (BCC_FUSED_PASS, bcc_set_fused_pass; round 6).
std::atomic<bool> g_fused_pass{[] {
    const char* e = getenv("BCC_FUSED_PASS");
    return !(e && atoi(e) == 0);
}()};

// Shards per worker of a long pass (BCC_LONG_SHARDS_PER_WORKER, bcc_set_long_shards_per_worker;
// default 1: one contiguous shard per worker).  With more, a worker that finishes early takes the
// next shard, so a worker on a slower (shared) core sets less of the pass's length.
std::atomic<unsigned> g_long_shards{[] {
    const char* e = getenv("BCC_LONG_SHARDS_PER_WORKER");
    return e ? (unsigned)std::max(1, atoi(e)) : 1u;
}()};

// Early Q halves for a single-GPU, single-chunk call (EarlyShard): per shard the candidates of its
// active items, then one early launch over all shards' rows (concatenated in shard order).
// Whether a chunk of n items takes early Q halves (its candidates are extracted by prepare).
bool early_wanted(size_t n, bool allow) {
    return allow && g_early_q.load(std::memory_order_relaxed) && device_list().size() == 1 &&
           n <= EARLY_MAX_ITEMS && n > host_small_round();
}

void chunk_early(ChunkRun& c, bool allow) {
    for (unsigned t = 0; t < c.T; t++) {
        c.rds[t].early = nullptr;
        c.rds[t].erow0 = 0;
        c.rds[t].early_mapped = 0;
        c.rds[t].early_msgs = 0;
    }
    const std::vector<int> devs = device_list();
    // the calling thread's device batches forget any early set of an earlier call or chunk first:
    // only a launch below may make one live again (Round::early gates its use today; the reset
    // keeps a future path that stages rows without that gate from reading a stale set)
    for (int d : devs) gpu_early_reset(d);
    if (!early_wanted(c.n, allow)) return;
    auto e0 = clk::now();
    std::vector<const TupleRows*> parts(c.T);
    size_t E = 0;
    std::vector<const SighashJobs*> jparts(c.T);
    for (unsigned t = 0; t < c.T; t++) {
        c.rds[t].erow0 = (uint32_t)E;
        E += c.early[t].rows.size();
        parts[t] = &c.early[t].rows;
        jparts[t] = &c.early[t].jobs;
    }
    if (E > host_small_round() && gpu_early_launch(devs[0], parts.data(), c.T, jparts.data()) == 0) {
        for (unsigned t = 0; t < c.T; t++) c.rds[t].early = &c.early[t];
        t_stats.early_rows += E;
    }
    t_stats.early_seconds += since(e0);
}

// prepare + shards + the first interpreter pass of items [0, n) of `items`.
void chunk_start(ChunkRun& c, const bcc_batch_item* items, size_t n, unsigned flags,
                 bool allow_early = false) {
    auto t0 = clk::now();
    c.n = n;
    // A short host pass (a block-sized batch) on at most the CPU share (C3 at 48 threads vs 16:
    // 2.9-3.0 vs 4.7-5.4 M inputs/s, profiles/r04/c3); round 5 made the share the default for
    // every pass (host_threads()), an explicit bcc_set_host_threads above it still applies to long
    // passes only.
    const unsigned cap = n < SHORT_PASS_ITEMS ? std::min(host_threads(), cpu_share()) : host_threads();
    c.W = n >= 256 ? std::min<unsigned>(cap, (unsigned)(n / 64)) : 1u;
    // shards per worker, dealt dynamically (run_shards): SHARDS_PER_WORKER for a short pass,
    // g_long_shards for a long one (bcc_set_long_shards_per_worker)
    const unsigned spw = n < SHORT_PASS_ITEMS ? SHARDS_PER_WORKER : g_long_shards.load(std::memory_order_relaxed);
    c.T = c.W > 1 ? std::min<unsigned>(std::max(1u, spw) * c.W, (unsigned)(n / 64)) : c.W;
    const unsigned T = c.T;
    const bool early = early_wanted(n, allow_early);
    if (early && c.early.size() < T) c.early.resize(T);
    auto round_state = [&] {  // per-shard state of the call (before its first interpreter pass)
        c.next_list.resize(T);
        for (auto& v : c.next_list) v.clear();
        if (c.rds.size() < T) c.rds.resize(T);
        for (unsigned t = 0; t < T; t++) {
            c.rds[t].keys.clear();
            c.rds[t].touched.clear();  // pointers into a previous call's tx entries: never followed
            c.rds[t].host_rejected = 0;
            c.rds[t].key_hashes = 0;
        }
        c.row0.assign(T + 1, 0);
        c.stage_s = 0;
        c.devices_used = 0;
        c.retries = 0;
    };
    // Round 6: without early Q halves (every pipelined chunk) the first interpreter pass runs
    // inside the parse pass, block by block per shard (prepare's FusedPass): each item is
    // interpreted while its tx bytes and parsed entry are still in cache, instead of in a second
    // pass over the whole chunk.  (The prepared HASH160s the pass reads exist only with
    // BCC_DEVICE_KEY_HASH=0, which keeps the two passes.)
    if (!early && g_fused_pass.load(std::memory_order_relaxed) &&
        g_device_key_hash.load(std::memory_order_relaxed)) {
        round_state();
        chunk_early(c, false);  // (resets the early pointers and the device's early sets)
        c.host_planned->store(0, std::memory_order_relaxed);
        for (unsigned t = 0; t < T; t++) {
            c.rds[t].reset(true);
            c.rds[t].host.planned = c.host_planned.get();
        }
        std::vector<char> ran(T, 0);
        std::vector<double> ts(T, 0);
        const FusedPass pass = [&](unsigned t, const uint32_t* idx, size_t m) {
            auto s0 = clk::now();
            ran[t] |= interpret_items(c.b, idx, m, c.rds[t]) ? 1 : 0;
            ts[t] += since(s0);
        };
        // a pipelined chunk's rows go to its staged batch shard by shard as the pass finishes them
        // (DeviceBatch::pre_upload), so its round's K_keyq need not wait for their upload
        std::function<void(unsigned)> sent;
        const std::function<void(unsigned)>* done = nullptr;
        if (c.pipelined && g_pre_upload.load(std::memory_order_relaxed) && direct_upload()) {
            const std::vector<int> devs = device_list();
            if (devs.size() == 1 && n > host_small_round()) {
                if (!c.staged) c.staged.reset(gpu_staged_new(devs[0]));
                const size_t cap = 2 * ((n + T - 1) / T) + 4096;  // rows per shard (more: the round sends them)
                if (gpu_staged_pre_arm(c.staged.get(), T, cap) == 0) {
                    sent = [&](unsigned t) { gpu_staged_pre_upload(c.staged.get(), t, c.rds[t].rows); };
                    done = &sent;
                }
            }
        }
        prepare(c.b, items, n, flags, T, &c.shards, &c.run_list, nullptr, c.W, &pass, done);
        double tmax = 0;
        for (double x : ts) tmax = std::max(tmax, x);
        const double both = since(t0);  // parse + interpret, split by the slowest shard's share
        t_stats.interpret_seconds += std::min(tmax, both);
        t_stats.prepare_seconds += both - std::min(tmax, both);
        chunk_interpret_finish(c, ran, ts);
        return;
    }
    prepare(c.b, items, n, flags, T, &c.shards, &c.run_list, early ? &c.early : nullptr, c.W);  // + the shard / run lists
    t_stats.prepare_seconds += since(t0);
    round_state();
    chunk_early(c, allow_early);
    chunk_interpret(c);
}

// Pipelined chunks: the caller stages the chunk's first device round into the chunk's own device
// batch with its whole team (the pinned image fill), so the pipeline worker only uploads, launches
// and waits.  Staged on the worker instead, the fill ran on a few threads beside the next chunk's
// host pass, which holds the CPU quota (stage 4.3 -> 7.4-9 ms per 1M inputs, profiles/r04/pipeline).
// Single-GPU rounds that go to the device as one batch only; anything else keeps the general path.
void prestage_round(ChunkRun& c) {
    c.prestaged = false;
    const std::vector<int> devs = device_list();
    if (devs.size() != 1 || c.row0[c.T] <= host_small_round()) return;
    size_t sz[5] = {0, 0, 0, 0, 0};
    std::vector<const SighashJobs*> pj;
    std::vector<const TupleRows*> pr;
    for (unsigned t = 0; t < c.T; t++) {
        const SighashJobs& j = c.rds[t].jobs;
        const size_t add[5] = {j.aux.size(), j.pre.size(), j.tpl.size(), j.code.size(), j.txraw.size()};
        for (int k = 0; k < 5; k++) sz[k] += add[k];
        pj.push_back(&j);
        pr.push_back(&c.rds[t].rows);
    }
    for (int k = 0; k < 5; k++)
        if (sz[k] > ROUND_BLOB_LIMIT) return;
    if (!c.staged) c.staged.reset(gpu_staged_new(devs[0]));
    double st = 0;
    struct StageThreads {  // a memory-bound fill: more threads than CPUs only add CPU time
        StageThreads() { set_stage_threads(cpu_share()); }
        ~StageThreads() { set_stage_threads(0); }
    } share_threads;
    if (gpu_staged_stage(c.staged.get(), pj.data(), pr.data(), pj.size(), &st) != 0) return;
    t_stats.stage_seconds += st;
    c.prestaged = true;
}

// Round 5: a prestaged round without late host jobs is queued on the GPU by the caller right
// after its staging (upload + kernels, non-blocking), so the next chunk's upload runs beside the
// previous chunk's kernels instead of after them; chunk_device_round then only waits for it.
void chunk_launch(ChunkRun& c) {
    c.launched = false;
    if (!c.prestaged || c.late_pending) return;
    if (take_injected_fault() != 0 || gpu_staged_launch(c.staged.get(), nullptr) != 0) {
        c.prestaged = false;  // the general path (retry, failure policy) runs it
        c.retries++;
        return;
    }
    c.prestaged = false;
    c.launched = true;
}

// The chunk's pending device round (its arguments stay valid until the chunk's next pass).
int chunk_device_round(ChunkRun& c) {
    LateHost* late = c.late_pending ? &c.late : nullptr;
    if (c.launched) {
        c.launched = false;
        const int e = gpu_staged_finish(c.staged.get(), c.verdict.data());
        if (e == 0) {
            c.devices_used = std::max<size_t>(c.devices_used, 1);
            return 0;
        }
        fprintf(stderr, "[bcc] verify_batch: staged device round failed (hip error %d): running it "
                        "again through the general path\n", e);
        c.retries++;
    } else if (c.prestaged) {
        c.prestaged = false;
        int e = take_injected_fault();
        if (!e) {
            const LateMsgFill fill = [&](std::vector<uint32_t>& rows, std::vector<uint8_t>& digs) {
                late->ensure();
                late_rows(c.rds, c.row0, 0, c.T, rows, digs);
            };
            e = gpu_staged_run(c.staged.get(), c.verdict.data(), late ? &fill : nullptr);
        }
        if (e == 0) {
            c.devices_used = std::max<size_t>(c.devices_used, 1);
            return 0;
        }
        fprintf(stderr, "[bcc] verify_batch: staged device round failed (hip error %d): running it "
                        "again through the general path\n", e);
        c.retries++;
    }
    struct StageW {  // more shards (staging parts) than workers: fill the image on the workers only
        explicit StageW(const ChunkRun& c) : on(c.T > c.W) {
            if (on) set_stage_threads(c.W);
        }
        ~StageW() {
            if (on) set_stage_threads(0);
        }
        bool on;
    } stage_w(c);
    return run_device_round(c.rds, c.T, c.row0, c.verdict.data(), &c.stage_s, &c.devices_used,
                            &c.retries, &c.host_rounds, late);
}

// Stitches a device round's verdicts into the items; the items whose speculation failed get
// another interpreter pass (their run lists).  Only those items' check caches receive the
// round's verdicts (round 6): an item whose consulted checks all came back true is final, and
// its cache is never read again in this call, so the common case touches each item once.
void chunk_stitch(ChunkRun& c) {
    auto& st = c.b.st;
    run_shards(c.T, c.W, [&](unsigned t) {
        const uint8_t* v = c.verdict.data() + c.row0[t];
        c.next_list[t].clear();
        // every row of this shard's round true (the common case): every speculation held and no
        // item of the shard re-runs -- one scan of the verdict bytes instead of a pass over items
        const size_t nr = c.row0[t + 1] - c.row0[t];
        if (nr == 0 || memchr(v, 0, nr) == nullptr) {
            c.run_list[t].clear();
            return;
        }
        for (uint32_t i : c.run_list[t]) {
            Item& it = st[i];
            if (it.pending.empty()) continue;
            bool all_true = true;
            for (uint32_t k : it.pending) all_true &= v[k] != 0;
            if (!all_true) {  // speculation was wrong somewhere: re-run with what the round learned
                // every check this item deferred in this round (consulted or a multisig
                // candidate hint) is still encoded as -2 - row; earlier rounds' are resolved
                for (Item::Check& ch : it.cache)
                    if (ch.v <= -2) ch.v = v[(uint32_t)(-2 - ch.v)] ? 1 : 0;
                it.active = true;
                c.next_list[t].push_back(i);
            }
        }
        c.run_list[t].swap(c.next_list[t]);
    });
}

// Completes the chunk: waits for (or runs) its device rounds, re-runs items until every run is
// final, writes ret / err.  `async`: device rounds go to the pipeline worker.  Returns the valid
// count, or -1 if a device round failed twice (those items get BCC_ERR_DEVICE_FAILURE).
long chunk_finish(ChunkRun& c, int* ret_out, bitcoinconsensus_error* err_out, bool async,
                  double* gpu_s) {
    auto& st = c.b.st;
    long status = 0;
    while (c.pending_round) {
        auto g0 = clk::now();
        const double p0 = process_cpu();
        int e;
        if (c.fut.valid()) {
            e = c.fut.get();
        } else if (async && !c.launched) {
            e = run_async([&c] { return chunk_device_round(c); }).get();
        } else {
            e = chunk_device_round(c);
        }
        *gpu_s += since(g0);
        t_stats.process_cpu_in_gpu_wait_seconds += process_cpu() - p0;
        t_stats.host_jobs_seconds += c.late.seconds;  // hashed during the round, maybe on a worker
        c.late.seconds = 0;
        t_stats.stage_seconds += c.stage_s;
        t_stats.device_retries += c.retries;
        t_stats.host_rounds += c.host_rounds;
        t_stats.devices = std::max(t_stats.devices, c.devices_used);
        c.stage_s = 0;
        c.retries = 0;
        c.host_rounds = 0;
        c.pending_round = false;
        if (e != 0) {
            status = -1;
            for (unsigned t = 0; t < c.T; t++)
                for (uint32_t i : c.run_list[t]) {
                    Item& it = st[i];
                    if (it.pending.empty()) continue;  // this run consulted no deferred check
                    it.result = false;
                    it.err = (bitcoinconsensus_error)BCC_ERR_DEVICE_FAILURE;
                    it.pending.clear();
                }
            break;
        }
        auto s1 = clk::now();
        chunk_stitch(c);
        t_stats.stitch_seconds += since(s1);
        bool rerun = false;  // every speculation held (the common case): no further pass at all
        for (unsigned t = 0; t < c.T; t++) rerun |= !c.run_list[t].empty();
        if (rerun) chunk_interpret(c);
    }
    for (unsigned t = 0; t < c.T; t++) {
        t_stats.host_rejected += c.rds[t].host_rejected;
        t_stats.device_key_hashes += c.rds[t].key_hashes;
        t_stats.early_mapped += c.rds[t].early_mapped;
        t_stats.early_msgs += c.rds[t].early_msgs;
    }
    auto f0 = clk::now();
    std::vector<long> vt(c.T, 0);
    run_shards(c.T, c.W, [&](unsigned t) {  // the shards cover [0, n) contiguously
        long v = 0;
        for (uint32_t i : c.shards[t]) {
            Item& it = st[i];
            int ret = (it.err == bitcoinconsensus_ERR_OK && it.result) ? 1 : 0;
            ret_out[i] = ret;
            if (err_out) err_out[i] = it.err;
            v += ret;
        }
        vt[t] = v;
    });
    long valid = 0;
    for (long v : vt) valid += v;
    t_stats.finish_seconds += since(f0);
    return status < 0 ? -1 : valid;
}

// The state stays with the calling thread for its next call, except after a very large chunk:
// then it is released, in parallel (freeing from one thread costs more than the interpreter pass
// itself).
void chunk_release_if_large(ChunkRun& c) {
    if (c.n <= ((size_t)1 << 22)) return;
    auto& st = c.b.st;
    run_shards(c.T, c.W, [&](unsigned t) {
        for (uint32_t i : c.shards[t]) {
            decltype(st[i].cache)().swap(st[i].cache);
            std::vector<uint32_t>().swap(st[i].pending);
        }
        c.rds[t] = Round();
        const size_t E = c.b.txs.size();  // every entry, not only this call's
        for (size_t k = share_lo(E, t, c.T); k < share_lo(E, t + 1, c.T); k++) c.b.txs[k].tx = Tx();
    });
    c.b = BatchState();
    c.rds = std::vector<Round>();
}

// Round 5: stage and queue a pipelined chunk's device round before waiting for the previous chunk
// (BCC_CHUNK_LAUNCH_EARLY=0: the round-4 order, staged after that wait and run on the worker).
const bool g_chunk_launch_early = [] {
    const char* e = getenv("BCC_CHUNK_LAUNCH_EARLY");
    return e ? atoi(e) != 0 : true;
}();

// Items per pipelined chunk (bcc_set_pipeline_chunk, BCC_PIPELINE_CHUNK; 0 disables pipelining).
// Round 4: chunk k's device round on the pipeline worker beside chunk k + 1's host pass, default
// 500000 items: 1M C2 inputs 24.9-25.2 -> 28.1-28.5 M inputs/s sustained over 10-call runs on the
// GPU box (profiles/r04/pipeline).  Rounds 2-3 measured pipelining as a loss; the cause was two
// per-chunk costs of the host pass, not interference from the device thread (a CPU-only probe
// with a sleeping device stub reproduced it, tools/pipe_probe): an interpreter pass over every
// shard after each device round even when no item needed a re-run (Round::reset walks every
// touched tx), and the per-item state shrinking and re-growing between chunks of different
// sizes (every Item's / TxEntry's buffers freed and re-allocated).  Both are gone.
std::atomic<size_t> g_pipeline_chunk{[] {
    const char* e = getenv("BCC_PIPELINE_CHUNK");
    return e ? (size_t)atoll(e) : (size_t)500000;
}()};
size_t pipeline_chunk() { return g_pipeline_chunk.load(std::memory_order_relaxed); }

// Items of a pipelined batch's last chunk (BCC_PIPELINE_TAIL; 0: the remainder, the round-5 cut).
// Round 6: the last chunk's device round (upload + kernels) is the only one that no host pass
// overlaps; 1M C2 inputs are cut 500k / 250k / 250k instead of 500k / 500k.
std::atomic<size_t> g_pipeline_tail{[] {
    const char* e = getenv("BCC_PIPELINE_TAIL");
    return e ? (size_t)atoll(e) : (size_t)0;
}()};
size_t pipeline_tail() { return g_pipeline_tail.load(std::memory_order_relaxed); }

// Staging threads of a pipelined device round: it fills its pinned image beside the next chunk's
// host pass, which has the CPU share.
constexpr unsigned PIPELINE_STAGE_THREADS = 4;

// Runs the batch; fills ret/err per item.  Returns -1 if the device pipeline failed twice in a
// row for some round: the items that round left unfinished get ret 0 and BCC_ERR_DEVICE_FAILURE
// (never a consensus verdict); all other items carry their final results.
// Host work (deserialization, interpreter passes, job building) runs on up to host_threads()
// threads over whole-transaction shards; each round's deferred checks of all shards go to the GPU
// together.  A batch of at least two pipeline chunks is cut into chunks of whole transactions
// whose first device round runs on the pipeline worker while the host works on the next chunk
// (double-buffered: two chunk slots, the worker's own device batch).
long run_batch(const bcc_batch_item* items, size_t n, unsigned flags, int* ret_out,
               bitcoinconsensus_error* err_out) {
    t_stats = bcc_batch_stats{};
    t_kinds = bcc_sighash_kinds{};
    t_stats.items = n;
    double gpu_s = 0;
    auto t0 = clk::now();
    const double cpu0 = process_cpu();
    const size_t chunk = pipeline_chunk();
    long status = 0, valid = 0;
    auto account = [&](long r) {
        if (r < 0) status = -1;
        else valid += r;
    };
    // On every exit, exceptions included: no chunk slot of this thread may keep a device round in
    // flight (the worker would go on writing the slot's rounds and verdicts while the next call
    // reuses it, and that call's chunk_finish would take the stale future), nor a pending or
    // prestaged round of this call.
    struct DrainSlots {
        ~DrainSlots() {
            for (auto& c : tl_chunk) {
                if (c.fut.valid()) {
                    try {
                        c.fut.get();
                    } catch (...) {
                    }
                }
                if (c.launched) {  // queued on the GPU: let it finish before the slot is reused
                    std::vector<uint8_t> v(std::max<size_t>(1, c.npend));
                    (void)gpu_staged_finish(c.staged.get(), v.data());
                    c.launched = false;
                }
                c.pending_round = false;
                c.prestaged = false;
                c.late_pending = false;
            }
        }
    } drain;
    if (chunk == 0 || n < 2 * chunk) {
        ChunkRun& c = tl_chunk[0];
        c.pipelined = false;
        chunk_start(c, items, n, flags, true);
        account(chunk_finish(c, ret_out, err_out, false, &gpu_s));
        chunk_release_if_large(c);
    } else {
        // chunk boundaries between transactions (adjacent items of one tx stay together); the last
        // chunk is cut down to pipeline_tail() items: its device round is the one no host pass
        // hides, so a smaller one returns the call sooner
        std::vector<size_t> cut{0};
        const size_t tail = std::min(pipeline_tail(), chunk);
        while (cut.back() < n) {
            const size_t rem = n - cut.back();
            const size_t step = tail == 0 || rem > chunk + tail ? chunk : rem > tail ? rem - tail : rem;
            size_t e = std::min(n, cut.back() + step);
            while (e < n && items[e].tx_to == items[e - 1].tx_to) e++;
            cut.push_back(e);
        }
        ChunkRun* prev = nullptr;
        size_t prev_lo = 0;
        for (size_t k = 0; k + 1 < cut.size(); k++) {
            ChunkRun& c = tl_chunk[k & 1];
            c.pipelined = true;
            chunk_start(c, items + cut[k], cut[k + 1] - cut[k], flags);
            if (c.pending_round && g_chunk_launch_early) {
                // staged and queued before the previous chunk is waited for: its upload runs
                // beside the previous chunk's kernels (chunk_launch)
                prestage_round(c);
                chunk_launch(c);
            }
            if (prev) {
                account(chunk_finish(*prev, ret_out + prev_lo, err_out ? err_out + prev_lo : nullptr,
                                     true, &gpu_s));
            }
            if (c.pending_round && !c.launched) {
                if (!g_chunk_launch_early) prestage_round(c);  // the pinned image, with the caller's team
                c.fut = run_async([&c] {
                    set_stage_threads(PIPELINE_STAGE_THREADS);  // re-runs stage beside the host pass
                    return chunk_device_round(c);
                });
            }
            prev = &c;
            prev_lo = cut[k];
        }
        account(chunk_finish(*prev, ret_out + prev_lo, err_out ? err_out + prev_lo : nullptr, true,
                             &gpu_s));
        chunk_release_if_large(tl_chunk[0]);
        chunk_release_if_large(tl_chunk[1]);
    }
    t_stats.host_seconds = since(t0) - gpu_s;
    t_stats.gpu_seconds = gpu_s;
    t_stats.process_cpu_seconds = process_cpu() - cpu0;
    return status < 0 ? -1 : valid;
}

}  // namespace

size_t build_first_round(const bcc_batch_item* items, size_t n, unsigned flags, SighashJobs& jobs,
                         TupleRows& rows, std::vector<uint32_t>* tuple_item) {
    BatchState b;
    prepare(b, items, n, flags, 1);
    std::vector<Round> rds(1);
    Round& rd = rds[0];
    rd.reset();  // the engine's thresholds: long chains hashed on the host as in a live round
    std::atomic<uint64_t> planned{0};
    rd.host.planned = &planned;
    std::vector<uint32_t> all(n);
    for (size_t i = 0; i < n; i++) all[i] = (uint32_t)i;
    interpret_shard(b, all, rd);
    if (mark_host_rows(rds, 1)) hash_host_jobs(rds, 1);
    if (tuple_item) {
        tuple_item->clear();
        for (const auto& p : rd.pending) tuple_item->push_back(p.item);
    }
    jobs = std::move(rd.jobs);
    rows = std::move(rd.rows);
    rows.materialize();  // full y / msg rows for the bench and test consumers
    return rows.size();
}

size_t build_sighash_checks(const SighashCheck* checks, size_t n, SighashJobs& jobs,
                            TupleRows& rows) {
    jobs.clear();
    rows.clear();
    rows.msg_one = true;
    rows.y_unused = true;
    std::vector<TxEntry> txs(n);
    std::vector<TxEntry*> touched;
    std::vector<uint8_t> scratch;
    Bip143Job bip143;
    const uint8_t zero[32] = {0};
    uint8_t one[32] = {0};
    one[0] = 1;
    size_t cur = 0;  // adjacent checks with the same tx buffer share its entry, as a batch's items do
    for (size_t i = 0; i < n; i++) {
        const SighashCheck& c = checks[i];
        if (i == 0 || c.tx != checks[i - 1].tx || c.tx_len != checks[i - 1].tx_len) {
            cur = i;
            if (!c.tx || !parse_tx(c.tx, c.tx_len, txs[cur].tx)) return i;
        }
        if (c.nin >= txs[cur].tx.vin.size()) return i;
        if (c.sigversion != SIGVERSION_BASE && c.sigversion != SIGVERSION_WITNESS_V0) return i;
        bcc_batch_item in{nullptr, 0, c.amount, c.tx, (unsigned)c.tx_len, c.nin};
        const Bytes code(c.code, c.code + c.code_len);
        const uint32_t row = rows.add(0x02, zero, zero, zero, zero, one);
        add_sighash_job(jobs, txs[cur], in, code, (SigVersion)c.sigversion, c.hashtype, row, scratch,
                        bip143, touched);
    }
    t_kinds = bcc_sighash_kinds{};
    count_kinds(jobs, 0);
    return n;
}

// src's rows and jobs behind dst's, its records rebased to their place (pipeline.h PartBase /
// rebase: the rule DeviceBatch::stage_parts applies to the parts of a device round).
void append_round(SighashJobs& dst, TupleRows& drows, const SighashJobs& src,
                  const TupleRows& srows) {
    const PartBase base = part_base(part_extent(&dst, drows));
    auto cat = [](auto& a, const auto& b) { a.insert(a.end(), b.begin(), b.end()); };
    // b behind a, rebased by `by` (a base of one field, or all of them for a record)
    auto cat_rebased = [](auto& a, const auto& b, const auto& by) {
        const size_t at = a.size();
        a.resize(at + b.size());
        rebase_copy(a.data() + at, b.data(), b.size(), by);
    };
    cat(drows.tag, srows.tag);
    cat(drows.x, srows.x);
    cat(drows.y, srows.y);
    cat(drows.r, srows.r);
    cat(drows.s, srows.s);
    cat(drows.msg, srows.msg);
    cat(dst.aux, src.aux);
    cat(dst.pre, src.pre);
    cat_rebased(dst.aux_off, src.aux_off, base.aux_blk);
    cat(dst.aux_nblk, src.aux_nblk);
    cat_rebased(dst.pre_off, src.pre_off, base.pre_blk);
    cat(dst.pre_nblk, src.pre_nblk);
    cat_rebased(dst.pre_row, src.pre_row, base.row);
    cat_rebased(dst.patches, src.patches, base);
    cat(dst.tpl, src.tpl);
    cat(dst.code, src.code);
    cat_rebased(dst.tjobs, src.tjobs, base);
    cat(dst.txraw, src.txraw);
    cat_rebased(dst.wtx, src.wtx, base);
    dst.win_entries += src.win_entries;
    cat_rebased(dst.wjobs, src.wjobs, base);
    cat_rebased(dst.ljobs, src.ljobs, base);
    dst.n_single_bug += src.n_single_bug;
    dst.n_win_single += src.n_win_single;
}

}  // namespace host
}  // namespace bcc

using namespace bcc::host;

extern "C" {

int bitcoinconsensus_verify_script_with_amount(const unsigned char* scriptPubKey,
                                               unsigned int scriptPubKeyLen, int64_t amount,
                                               const unsigned char* txTo, unsigned int txToLen,
                                               unsigned int nIn, unsigned int flags,
                                               bitcoinconsensus_error* err) {
    bcc_batch_item item{scriptPubKey, scriptPubKeyLen, amount, txTo, txToLen, nIn};
    int ret = 0;
    bitcoinconsensus_error e = bitcoinconsensus_ERR_OK;
    long rc;
    try {
        rc = run_batch(&item, 1, flags, &ret, &e);
    } catch (...) {
        return set_err(err, bitcoinconsensus_ERR_TX_DESERIALIZE);
    }
    if (rc < 0) {
        // Only under BCC_DEVICE_FAILURE_ERROR (the default policy verifies a failed round on the
        // host): there is no verdict, and the reference ABI has no code for "no verdict" (every
        // error it reports is about the transaction, bitcoinconsensus.cpp:83-100).  Reporting 0
        // would reject a possibly valid spend as a consensus failure, so the call fails loudly
        // instead, as libsecp256k1's illegal-argument callback does (secp256k1.c:45-54).
        // bitcoinconsensus_verify_batch reports the same condition as -1.
        fprintf(stderr, "[bcc] bitcoinconsensus_verify_script_with_amount: GPU unavailable, no "
                        "verdict; aborting\n");
        abort();
    }
    // set_error semantics (bitcoinconsensus.cpp:58-63): errors return 0 and write *err;
    // a completed script run writes ERR_OK
    if (err) *err = e;
    return ret;
}

int bitcoinconsensus_verify_script(const unsigned char* scriptPubKey, unsigned int scriptPubKeyLen,
                                   const unsigned char* txTo, unsigned int txToLen,
                                   unsigned int nIn, unsigned int flags, bitcoinconsensus_error* err) {
    if (flags & bitcoinconsensus_SCRIPT_FLAGS_VERIFY_WITNESS)
        return set_err(err, bitcoinconsensus_ERR_AMOUNT_REQUIRED);
    return bitcoinconsensus_verify_script_with_amount(scriptPubKey, scriptPubKeyLen, 0, txTo,
                                                      txToLen, nIn, flags, err);
}

unsigned int bitcoinconsensus_version(void) { return BITCOINCONSENSUS_API_VER; }

long bitcoinconsensus_verify_batch(const bcc_batch_item* items, size_t n, unsigned int flags,
                                   int* ret_out, bitcoinconsensus_error* err_out) {
    bcc::host::ActiveCaller active;
    try {
        auto t0 = std::chrono::steady_clock::now();
        long r = run_batch(items, n, flags, ret_out, err_out);
        t_stats.total_seconds =
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return r;
    } catch (...) {
        for (size_t i = 0; i < n; i++) {
            ret_out[i] = 0;
            if (err_out) err_out[i] = bitcoinconsensus_ERR_TX_DESERIALIZE;
        }
        return -1;
    }
}

void bcc_debug_fail_device_rounds(int rounds) {
    g_fail_code.store(2);
    g_fail_rounds.store(rounds > 0 ? rounds : 0);
}

void bcc_debug_fail_device_rounds_code(int rounds, int hip_error) {
    g_fail_code.store(hip_error ? hip_error : 2);
    g_fail_rounds.store(rounds > 0 ? rounds : 0);
}

int bcc_set_device_key_hash(int on) {
    bcc::host::g_device_key_hash.store(on != 0, std::memory_order_relaxed);
    return 0;
}

int bcc_set_device_hashtypes(int on) {
    bcc::host::g_device_hashtypes.store(on != 0, std::memory_order_relaxed);
    return 0;
}

void bcc_last_sighash_kinds(bcc_sighash_kinds* out) {
    if (out) *out = t_kinds;
}

int bcc_set_host_chain_blocks(unsigned blocks) {
    bcc::host::g_host_chain_blocks.store(blocks, std::memory_order_relaxed);
    return 0;
}

int bcc_set_host_bip143_blocks(unsigned blocks) {
    bcc::host::g_host_bip143_blocks.store(blocks, std::memory_order_relaxed);
    return 0;
}

int bcc_set_early_q(int on) {
    bcc::host::g_early_q.store(on ? 1 : 0, std::memory_order_relaxed);
    return 0;
}

int bcc_set_pipeline_chunk(size_t items) {
    g_pipeline_chunk.store(items, std::memory_order_relaxed);
    return 0;
}

int bcc_set_pre_upload(int on) {
    bcc::host::g_pre_upload.store(on != 0, std::memory_order_relaxed);
    return 0;
}

int bcc_set_direct_upload(int on) {
    bcc::set_direct_upload(on != 0);
    return 0;
}

int bcc_set_fused_pass(int on) {
    g_fused_pass.store(on != 0, std::memory_order_relaxed);
    return 0;
}

int bcc_set_long_shards_per_worker(unsigned k) {
    if (k == 0 || k > 64) return -1;
    g_long_shards.store(k, std::memory_order_relaxed);
    return 0;
}

int bcc_set_pipeline_tail(size_t items) {
    g_pipeline_tail.store(items, std::memory_order_relaxed);
    return 0;
}

void bcc_release_thread_state(void) {
    for (auto& c : tl_chunk) c = ChunkRun();
    bcc::host::inputs_release_thread_state();
    bcc::host::taproot_release_thread_state();
    bcc::host::block_release_thread_state();
    bcc::release_device_thread_state();
    bcc::release_tuple_thread_state();
    bcc::host::release_pubkey_rows();
    bcc::host::release_team();
    // the state the per-GPU and pipeline workers keep for the rounds they ran for callers: only
    // when no other caller is inside an entry point (their rounds use it)
    if (bcc::host::other_active_callers() == 0) {
        bcc::host::run_on_all_workers([] {
            bcc::host::taproot_release_thread_state();
            bcc::host::block_release_thread_state();
            bcc::release_device_thread_state();
            bcc::release_tuple_thread_state();
            bcc::host::release_pubkey_rows();
            bcc::host::release_team();
        });
    }
    bcc::pinned_trim();  // the page-locked blocks no array holds any more
}

int bcc_set_device(int device) {
    std::lock_guard<std::mutex> lk(g_device_mu);
    g_device = device;
    return 0;
}

void bcc_last_batch_stats(bcc_batch_stats* out) {
    if (out) *out = t_stats;
}

}  // extern "C"
