// A block's transaction hashes and merkle commitments in batch: bcc_tx_hashes_batch,
// bcc_merkle_root, bcc_block_commitments_batch (include/bcc_amd.h).
//
// Host half: the block parser (header, canonical CompactSize count, parse_tx per transaction, exact
// length), GetWitnessCommitmentIndex and the shape of the coinbase's reserved value
// (consensus/validation.h:161-179, validation.cpp:3575-3610), one TxHashJob per transaction built
// per part on the calling thread's team and rebased into the round (pipeline.h BlockBase), the
// round loop, and the comparisons on the roots a round returns.  A round runs on the device
// through g_block_device_hook (block_hash.hip), or here on the host over the same records
// (block_round_host): rounds of at most the small-round threshold, and rounds the device could not
// deliver (the Taproot side's failure rules, taproot_host.h).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <vector>

#include "../block_hash.h"
#include "../block_rules.h"
#include "bcc_amd.h"
#include "bitcoinconsensus.h"
#include "block_entry.h"
#include "devices.h"
#include "engine.h"
#include "hashes.h"
#include "host_verify.h"
#include "taproot_host.h"
#include "team.h"
#include "tuples.h"
#include "tx.h"

namespace bcc {

const BlockDeviceHook* g_block_device_hook = nullptr;

namespace host {
namespace {

// Transactions per device round when bcc_set_block_round is 0.
constexpr size_t BLOCK_ROUND_TXS = (size_t)1 << 18;
// Raw bytes per round: the records' offsets are 32-bit, and the arena is uploaded in one copy.
constexpr size_t BLOCK_ROUND_BYTES = (size_t)1 << 30;
// A buffer the 32-bit records cannot index.
constexpr size_t BLOCK_MAX_BYTES = (size_t)1 << 31;
// Transactions per device share of a call with device = -1.
constexpr size_t DEVICE_SHARE_TXS = 256;

std::atomic<size_t> g_block_round{0};
// Provisional defaults: the entries' small-round threshold in transactions or
// leaves, and the long-chain threshold in 64-byte blocks.
#ifndef BCC_BLOCK_SMALL_ROUND
#define BCC_BLOCK_SMALL_ROUND 2048
#endif
#ifndef BCC_HOST_TXHASH_BLOCKS
#define BCC_HOST_TXHASH_BLOCKS 16
#endif
std::atomic<unsigned> g_host_txhash_blocks{BCC_HOST_TXHASH_BLOCKS};

// 0 with bcc_set_host_small_round(0); else the entries' own threshold, or the caller's larger one
size_t block_small_round() {
    const size_t s = host_small_round();
    return s ? std::max(s, (size_t)BCC_BLOCK_SMALL_ROUND) : 0;
}
size_t block_round_txs() {
    const size_t r = g_block_round.load(std::memory_order_relaxed);
    return r ? r : BLOCK_ROUND_TXS;
}

thread_local bcc_block_stats t_block_stats{};
thread_local double t_parse_ms = 0;  // bcc_block_last_timing_ms: the calling thread's parse clock

void reset_timing() {
    t_parse_ms = 0;
    if (g_block_device_hook) g_block_device_hook->timing_ms(nullptr, 1);
    if (g_block_rules_device_hook) g_block_rules_device_hook->timing_ms(nullptr, 1);
}
struct ParseClock {  // adds its lifetime to the calling thread's parse time
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~ParseClock() {
        t_parse_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
};

struct BlockCounters {
    std::atomic<size_t> blocks{0}, txs{0}, bytes{0}, long_txs{0}, merkle_launches{0};
    TaprootCounters t;  // rounds, host rounds, retries: what the failure rules count
    void store() const {
        bcc_block_stats s{};
        s.blocks = blocks.load();
        s.txs = txs.load();
        s.bytes_hashed = bytes.load();
        s.host_rounds = t.host_rounds.load();
        s.device_rounds = t.rounds.load() - s.host_rounds;
        s.host_long_txs = long_txs.load();
        s.merkle_launches = merkle_launches.load();
        s.device_retries = t.device_retries.load();
        t_block_stats = s;
    }
};

// message bytes of the SHA-256d's of a tree over n leaves (64 per parent)
size_t tree_bytes(size_t n) {
    size_t b = 0;
    for (; n > 1; n = (n + 1) / 2) b += 64 * ((n + 1) / 2);
    return b;
}
size_t job_bytes(const TxHashJob& j) { return txh_stripped_len(j) + (txh_w_lane(j) ? j.len : 0); }

// ---- the parser ------------------------------------------------------------------------------

// ReadCompactSize with range_check (serialize.h:318-347) at p[pos]; false where it throws.
bool read_compact(const uint8_t* p, size_t len, size_t& pos, uint64_t& v) {
    if (pos >= len) return false;
    const uint8_t c = p[pos++];
    const int k = c < 253 ? 0 : c == 253 ? 2 : c == 254 ? 4 : 8;
    if ((size_t)k > len - pos) return false;
    v = c;
    if (k) {
        v = 0;
        for (int i = k - 1; i >= 0; i--) v = (v << 8) | p[pos + i];
        pos += k;
        if (v < (k == 2 ? 253u : k == 4 ? 0x10000ull : 0x100000000ull)) return false;
    }
    return v <= 0x02000000;  // MAX_SIZE
}

// The record of a parsed transaction at tx (its first byte at `off` of its part); row and flags
// are the caller's.
TxHashJob tx_job(const Tx& t, const uint8_t* tx, size_t off) {
    TxHashJob j{};
    j.off = (uint32_t)off;
    j.len = (uint32_t)t.ser_size;
    if (t.has_witness()) {  // the extended format: marker, flag, at least one input
        const uint8_t* end = t.vout.empty() ? t.vin.back().script_sig.end() + 4 + 1
                                            : t.vout.back().ser.end();
        j.wit = (uint32_t)(end - tx);
    }
    return j;
}

// One block as its rounds need it.
struct ParsedBlock {
    int status = 0;  // 0, BCC_BLOCK_ERR_DESERIALIZE or BCC_BLOCK_ERR_EMPTY
    int commit_pos = -1;
    bool any_witness = false;
    bool commit_rule = false;  // segwit_active and a commitment output: rule 3's first branch
    bool nonce_ok = false;     // ... and the reserved value has its shape: the witness tree runs
    const uint8_t* commit32 = nullptr;  // scriptPubKey[6..38) of the last commitment output
    const uint8_t* nonce32 = nullptr;   // the reserved value
    size_t bytes = 0;                   // message bytes of its digests and trees
    std::vector<TxHashJob> jobs;        // off from the block's first byte, row = tx index
    std::vector<uint32_t> n_in;         // the rule entries: each transaction's input count
    void reset(int st) {  // (jobs keeps its capacity from call to call)
        status = st;
        commit_pos = -1;
        any_witness = commit_rule = nonce_ok = false;
        commit32 = nonce32 = nullptr;
        bytes = 0;
        jobs.clear();
        n_in.clear();
    }
};

void parse_block(const bcc_block_ref& b, ParsedBlock& P, Tx& tx, bool rules) {
    P.reset(BCC_BLOCK_ERR_DESERIALIZE);
    const uint8_t* p = b.block;
    const size_t len = b.block_len;
    if (len < 80 || len >= BLOCK_MAX_BYTES) return;
    size_t pos = 80;
    uint64_t count = 0;
    if (!read_compact(p, len, pos, count) || count > len - pos) return;
    P.jobs.reserve((size_t)count);
    for (uint64_t k = 0; k < count; k++) {
        if (!parse_tx(p + pos, len - pos, tx)) {
            P.reset(BCC_BLOCK_ERR_DESERIALIZE);
            return;
        }
        TxHashJob j = tx_job(tx, p + pos, pos);
        j.row = (uint32_t)k;
        P.any_witness |= j.wit != 0;
        if (k == 0) {  // the coinbase: GetWitnessCommitmentIndex and the reserved value
            for (size_t o = 0; o < tx.vout.size(); o++) {
                const Span& s = tx.vout[o].script;
                static const uint8_t head[6] = {0x6a, 0x24, 0xaa, 0x21, 0xa9, 0xed};
                if (s.n >= 38 && memcmp(s.p, head, 6) == 0) {
                    P.commit_pos = (int)o;
                    P.commit32 = s.p + 6;
                }
            }
            if (!tx.vin.empty() && tx.vin[0].witness.size() == 1 && tx.vin[0].witness[0].n == 32) {
                P.nonce_ok = true;
                P.nonce32 = tx.vin[0].witness[0].p;
            }
        }
        P.jobs.push_back(j);
        if (rules) P.n_in.push_back((uint32_t)tx.vin.size());
        pos += tx.ser_size;
    }
    if (pos != len) {
        P.reset(BCC_BLOCK_ERR_DESERIALIZE);
        return;
    }
    if (count == 0) {
        P.reset(BCC_BLOCK_ERR_EMPTY);
        return;
    }
    P.status = 0;
    P.commit_rule = b.segwit_active && P.commit_pos >= 0;
    P.nonce_ok = P.commit_rule && P.nonce_ok;
    if (P.nonce_ok) {  // the witness tree: every wtxid, the coinbase's as zero
        for (TxHashJob& j : P.jobs) j.flags = TXH_W;
        P.jobs[0].flags = TXH_W | TXH_WZERO;
    }
    P.bytes = tree_bytes(P.jobs.size()) * (P.nonce_ok ? 2 : 1) + (P.nonce_ok ? 64 : 0);
    for (const TxHashJob& j : P.jobs) P.bytes += job_bytes(j);
}

// ---- one round -------------------------------------------------------------------------------

// What the calling thread (or a device worker) keeps from round to round.
struct RoundState {
    std::vector<TxHashJob> jobs;
    std::vector<const uint8_t*> src;
    std::vector<MerkleSeg> segs;
    std::vector<uint8_t> txid, roots;
    std::vector<uint32_t> mut;
    std::vector<uint8_t> rows;  // block_round_host's node rows
    // the rule entries: input table rows per job (prefix sums), the blocks' contexts and results,
    // the jobs' records
    std::vector<uint32_t> in_base;
    std::vector<BlockRuleCtx> ctx;
    std::vector<BlockRuleOut> rule_out;
    std::vector<TxRuleRec> recs;
};
// rows of the input table: a transaction with one input cannot repeat an outpoint
uint32_t in_rows(uint32_t n_in) { return n_in >= 2 ? n_in : 0; }
thread_local RoundState tl_round;
thread_local std::vector<ParsedBlock> tl_blocks;

struct RangeState {
    int device;
    DeviceRange fail;
    BlockCounters& c;
};

// The round under the failure rules: on the host when it is small or cannot be indexed by the
// device records, else on the device with one retry and the policy.
int run_round(const char* who, BlockRound& r, size_t rows, bool device_ok, RangeState& rs) {
    auto on_host = [&] {
        block_round_host(r, host_threads());
        if (r.rules) block_rules_round_host(r);
    };
    if (!device_ok || rows <= block_small_round()) {
        on_host();
        rs.c.t.round(rows, 0, true);
        return 0;
    }
    const BlockDeviceHook* hook = g_block_device_hook;
    const int e = resilient_taproot_round(who, rs.device, rows, 0, rs.fail, rs.c.t, [&] {
        if (hook) return hook->round(rs.device, r);
        on_host();  // a build without the kernels
        return 0;
    }, on_host);
    if (e) return e;
    rs.c.long_txs += r.long_txs;
    rs.c.merkle_launches += r.merkle_launches;
    return 0;
}

// Blocks [lo, hi) of one device range, in rounds of whole blocks.
int blocks_range(const bcc_block_ref* blocks, const ParsedBlock* parsed, size_t lo, size_t hi,
                 bcc_block_result* out, RangeState& rs, const BlockRulesCall* rules) {
    RoundState& S = tl_round;
    const size_t round_txs = block_round_txs();
    for (size_t b0 = lo; b0 < hi;) {
        // the round's blocks: at least one, then while they fit
        size_t b1 = b0, n = 0, raw = 0;
        while (b1 < hi) {
            const size_t bn = parsed[b1].jobs.size(), bl = bn ? blocks[b1].block_len : 0;
            if (b1 > b0 && (n + bn > round_txs || raw + bl > BLOCK_ROUND_BYTES)) break;
            n += bn;
            raw += bl;
            b1++;
        }
        S.jobs.resize(n);
        S.src.resize(n);
        S.segs.clear();
        S.txid.resize(32 * n);
        S.roots.assign(64 * (b1 - b0), 0);
        S.mut.assign(2 * (b1 - b0), 0);
        S.ctx.clear();
        if (rules) S.in_base.assign(n + 1, 0);
        size_t row0 = 0, raw0 = 0;
        for (size_t b = b0; b < b1; b++) {
            const ParsedBlock& P = parsed[b];
            const size_t bn = P.jobs.size();
            if (bn == 0) continue;
            rebase_copy(&S.jobs[row0], P.jobs.data(), bn, BlockBase{(uint32_t)raw0, (uint32_t)row0});
            for (size_t k = 0; k < bn; k++) S.src[row0 + k] = blocks[b].block + P.jobs[k].off;
            const uint32_t t = (uint32_t)(2 * (b - b0));
            S.segs.push_back(MerkleSeg{(uint32_t)row0, (uint32_t)bn, 0, t});
            if (P.nonce_ok) S.segs.push_back(MerkleSeg{(uint32_t)(n + row0), (uint32_t)bn, 0, t + 1});
            if (rules) {
                BlockRuleCtx c = rules->ctx(b);
                c.job0 = 0;
                c.n_tx = (uint32_t)bn;
                rebase(c, BlockRuleBase{(uint32_t)row0});
                S.ctx.push_back(c);
                for (size_t k = 0; k < bn; k++)
                    S.in_base[row0 + k + 1] = S.in_base[row0 + k] + in_rows(P.n_in[k]);
            }
            row0 += bn;
            raw0 += blocks[b].block_len;
        }
        if (n) {
            BlockRound r;
            r.jobs = S.jobs.data();
            r.src = S.src.data();
            r.n_jobs = r.rows = n;
            r.raw_bytes = raw;
            r.host_blocks = g_host_txhash_blocks.load(std::memory_order_relaxed);
            r.segs = S.segs.data();
            r.n_segs = S.segs.size();
            r.n_trees = 2 * (b1 - b0);
            r.txid = S.txid.data();
            r.roots = S.roots.data();
            r.mut = S.mut.data();
            BlockRulesRound q;
            if (rules) {
                S.rule_out.assign(S.ctx.size(), BlockRuleOut{});
                q.in_base = S.in_base.data();
                q.ctx = S.ctx.data();
                q.n_blocks = S.ctx.size();
                q.out = S.rule_out.data();
                r.rules = &q;
            }
            if (int e = run_round(rules ? "block_check_batch" : "block_commitments_batch", r, n,
                                  raw < BLOCK_MAX_BYTES, rs))
                return e;
        }
        // the comparisons, in Core's order
        row0 = 0;
        size_t kb = 0;  // the blocks of the round that have transactions
        for (size_t b = b0; b < b1; b++) {
            const ParsedBlock& P = parsed[b];
            bcc_block_result& R = out[b];
            memset(&R, 0, sizeof R);
            R.status = P.status;
            R.commit_pos = -1;
            rs.c.blocks++;
            if (P.status) {
                if (rules) rules->block(b, R, nullptr);
                continue;
            }
            const size_t bn = P.jobs.size();
            const uint8_t* root = &S.roots[64 * (b - b0)];
            R.n_tx = (unsigned)bn;
            R.commit_pos = P.commit_pos;
            memcpy(R.merkle_root, root, 32);
            if (P.nonce_ok) memcpy(R.witness_root, root + 32, 32);
            if (blocks[b].txid_out && blocks[b].txid_cap >= bn)
                memcpy(blocks[b].txid_out, &S.txid[32 * row0], 32 * bn);
            rs.c.txs += bn;
            rs.c.bytes += P.bytes;
            row0 += bn;
            if (memcmp(root, blocks[b].block + 36, 32) != 0) {
                R.status = BCC_BLOCK_ERR_MERKLE_ROOT;
            } else if (S.mut[2 * (b - b0)]) {
                R.status = BCC_BLOCK_ERR_DUPLICATE;
            } else if (P.commit_rule) {
                uint8_t m[64], h[32];
                if (!P.nonce_ok) {
                    R.status = BCC_BLOCK_ERR_WITNESS_NONCE_SIZE;
                } else {
                    memcpy(m, root + 32, 32);
                    memcpy(m + 32, P.nonce32, 32);
                    sha256d(m, 64, h);
                    if (memcmp(h, P.commit32, 32) != 0) R.status = BCC_BLOCK_ERR_WITNESS_MERKLE;
                }
            } else if (P.any_witness) {
                R.status = BCC_BLOCK_ERR_UNEXPECTED_WITNESS;
            }
            if (rules) rules->block(b, R, &S.rule_out[kb++]);
        }
        b0 = b1;
    }
    return 0;
}

// Items [lo, hi) of bcc_tx_hashes_batch on one device, in rounds of item ranges.  The parts of a
// round (one team thread's share each) parse their items and count bytes and rows from zero.
struct TxPart {
    std::vector<TxHashJob> jobs;
    std::vector<const uint8_t*> src;
    std::vector<uint32_t> n_in;  // the rule entries: each job's input count
    size_t raw = 0;
};
thread_local std::vector<TxPart> tl_tx_parts;

int tx_range(const bcc_tx_ref* items, size_t lo, size_t hi, uint8_t* txid_out, uint8_t* wtxid_out,
             int* err_out, RangeState& rs, const BlockRulesCall* rules) {
    RoundState& S = tl_round;
    const size_t round_txs = block_round_txs();
    for (size_t r0 = lo; r0 < hi;) {
        size_t r1 = r0, raw = 0;
        while (r1 < hi && r1 - r0 < round_txs && (r1 == r0 || raw + items[r1].tx_len <= BLOCK_ROUND_BYTES))
            raw += items[r1++].tx_len;
        const size_t m = r1 - r0;
        const unsigned T = pool_threads(m, 256);
        std::vector<TxPart>& parts = tl_tx_parts;
        if (parts.size() < T) parts.resize(T);
        auto clock = std::make_unique<ParseClock>();
        run_team(T, [&](unsigned t) {
            TxPart& P = parts[t];
            P.jobs.clear();
            P.src.clear();
            P.n_in.clear();
            P.raw = 0;
            Tx tx;
            const size_t a = r0 + m * t / T, b = r0 + m * (t + 1) / T;
            for (size_t i = a; i < b; i++) {
                int e = 0;
                if (!parse_tx(items[i].tx, items[i].tx_len, tx)) e = bitcoinconsensus_ERR_TX_DESERIALIZE;
                else if (tx.ser_size != items[i].tx_len) e = bitcoinconsensus_ERR_TX_SIZE_MISMATCH;
                if (err_out) err_out[i] = e;
                if (e && rules) rules->tx(i, e, nullptr);
                if (e) {  // no record: the rows stay zero
                    if (txid_out) memset(txid_out + 32 * i, 0, 32);
                    if (wtxid_out) memset(wtxid_out + 32 * i, 0, 32);
                    continue;
                }
                TxHashJob j = tx_job(tx, items[i].tx, P.raw);
                j.row = (uint32_t)(i - a);
                j.flags = wtxid_out ? TXH_W : 0;
                P.jobs.push_back(j);
                P.src.push_back(items[i].tx);
                if (rules) P.n_in.push_back((uint32_t)tx.vin.size());
                P.raw += items[i].tx_len;
            }
        });
        clock.reset();
        size_t n = 0;
        for (unsigned t = 0; t < T; t++) n += parts[t].jobs.size();
        S.jobs.resize(n);
        S.src.resize(n);
        size_t k0 = 0, raw0 = 0, bytes = 0;
        if (rules) S.in_base.assign(n + 1, 0);
        for (unsigned t = 0; t < T; t++) {
            const TxPart& P = parts[t];
            for (size_t k = 0; rules && k < P.jobs.size(); k++)
                S.in_base[k0 + k + 1] = S.in_base[k0 + k] + in_rows(P.n_in[k]);
            rebase_copy(S.jobs.data() + k0, P.jobs.data(), P.jobs.size(),
                        BlockBase{(uint32_t)raw0, (uint32_t)(m * t / T)});
            std::copy(P.src.begin(), P.src.end(), S.src.begin() + k0);
            k0 += P.jobs.size();
            raw0 += P.raw;
        }
        for (const TxHashJob& j : S.jobs) bytes += job_bytes(j);
        if (n) {
            BlockRound r;
            r.jobs = S.jobs.data();
            r.src = S.src.data();
            r.n_jobs = n;
            r.rows = m;
            r.raw_bytes = raw0;
            r.host_blocks = g_host_txhash_blocks.load(std::memory_order_relaxed);
            // rows are the round's items: a row without a record is not written by the round
            S.txid.resize(32 * m);
            r.txid = txid_out ? txid_out + 32 * r0 : S.txid.data();
            r.wtxid = wtxid_out ? wtxid_out + 32 * r0 : nullptr;
            BlockRulesRound q;
            if (rules) {
                S.recs.assign(n, TxRuleRec{});
                q.in_base = S.in_base.data();
                q.recs = S.recs.data();
                r.rules = &q;
            }
            if (int e = run_round(rules ? "tx_check_batch" : "tx_hashes_batch", r, n,
                                  raw0 < BLOCK_MAX_BYTES, rs))
                return e;
            for (size_t k = 0; rules && k < n; k++) rules->tx(r0 + S.jobs[k].row, 0, &S.recs[k]);
        }
        rs.c.txs += n;
        rs.c.bytes += bytes;
        r0 = r1;
    }
    return 0;
}

// Contiguous shares of [0, n) by weight over the configured devices (device = -1) or the one.
int over_devices(int device, const std::vector<size_t>& weight,
                 const std::function<int(int, size_t, size_t)>& f) {
    ActiveCaller active;
    std::vector<int> devs = device < 0 ? device_list() : std::vector<int>{device};
    size_t total = 0;
    for (size_t w : weight) total += w;
    const size_t D = std::max<size_t>(
        1, std::min<size_t>({devs.size(), weight.size(), (total + DEVICE_SHARE_TXS - 1) / DEVICE_SHARE_TXS}));
    const std::vector<size_t> cut = split_balanced(weight, D);
    std::vector<std::function<int()>> jobs;
    std::vector<int> used;
    for (size_t d = 0; d + 1 < cut.size(); d++) {
        const size_t lo = cut[d], hi = cut[d + 1];
        if (lo >= hi) continue;
        const int dev = devs[d];
        used.push_back(dev);
        jobs.push_back([=, &f] { return f(dev, lo, hi); });
    }
    return jobs.empty() ? 0 : run_on_devices(used, jobs);
}

}  // namespace

// ---- the host evaluation ---------------------------------------------------------------------

void tx_hash_job_host(const TxHashJob& j, const uint8_t* tx, uint8_t* txid_rows, uint8_t* wtxid_rows) {
    uint8_t* t = txid_rows + 32 * (size_t)j.row;
    if (j.wit) {
        uint8_t d[32];
        Sha256 h;
        h.write(tx, 4).write(tx + 6, j.wit - 6).write(tx + j.len - 4, 4);
        h.finalize(d);
        sha256(d, 32, t);
    } else {
        sha256d(tx, j.len, t);
    }
    if (!wtxid_rows || !(j.flags & (TXH_W | TXH_WZERO))) return;
    uint8_t* w = wtxid_rows + 32 * (size_t)j.row;
    if (j.flags & TXH_WZERO) memset(w, 0, 32);
    else if (j.wit) sha256d(tx, j.len, w);
    else memcpy(w, t, 32);
}

bool merkle_root_host(const uint8_t* leaves, size_t n, uint8_t* root32, bool team) {
    thread_local std::vector<uint8_t> scratch;  // two level buffers (a team thread keeps its own)
    const size_t half = 32 * ((n + 1) / 2);
    if (scratch.size() < 2 * half) scratch.resize(2 * half);
    std::atomic<bool> mutated{false};
    const uint8_t* cur = leaves;
    int side = 0;
    while (n > 1) {
        const size_t m = (n + 1) / 2;
        uint8_t* out = scratch.data() + (side ? half : 0);
        auto parents = [&](size_t lo, size_t hi) {
            for (size_t k = lo; k < hi; k++) {
                const uint8_t* l = cur + 64 * k;
                if (2 * k + 1 < n) {
                    if (memcmp(l, l + 32, 32) == 0) mutated.store(true, std::memory_order_relaxed);
                    sha256d(l, 64, out + 32 * k);
                } else {  // an odd level's last node, paired with itself
                    uint8_t two[64];
                    memcpy(two, l, 32);
                    memcpy(two + 32, l, 32);
                    sha256d(two, 64, out + 32 * k);
                }
            }
        };
        if (team) pfor(m, 128, parents);
        else parents(0, m);
        cur = out;
        n = m;
        side ^= 1;
    }
    memcpy(root32, cur, 32);
    return mutated.load();
}

void block_round_host(BlockRound& r, unsigned threads) {
    RoundState& S = tl_round;
    r.long_txs = r.merkle_launches = 0;
    const uint8_t* nodes = r.leaves;
    if (!r.leaves) {
        // the node rows: the round's own when trees read them, else the caller's arrays (the rows
        // no job names were zeroed by the caller)
        uint8_t *trow = r.txid, *wrow = r.wtxid;
        if (r.n_segs) {
            S.rows.resize(64 * r.rows);
            trow = S.rows.data();
            wrow = trow + 32 * r.rows;
        }
        pfor(r.n_jobs, 64, [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; i++) tx_hash_job_host(r.jobs[i], r.src[i], trow, wrow);
        });
        if (r.n_segs && r.txid) memcpy(r.txid, trow, 32 * r.rows);
        nodes = trow;
    }
    // many trees: one per team thread at a time; few: each tree's levels over the team
    const bool across = r.n_segs >= 2 * (size_t)std::max(1u, threads);
    auto tree = [&](const MerkleSeg& m, bool team) {
        if (m.n_in == 0) return;
        r.mut[m.seg] = merkle_root_host(nodes + 32 * (size_t)m.base, m.n_in,
                                        r.roots + 32 * (size_t)m.seg, team) ? 1u : 0u;
    };
    if (across) {
        pfor(r.n_segs, 1, [&](size_t lo, size_t hi) {
            for (size_t s = lo; s < hi; s++) tree(r.segs[s], false);
        });
    } else {
        for (size_t s = 0; s < r.n_segs; s++) tree(r.segs[s], true);
    }
}

void block_release_thread_state() {
    tl_round = RoundState();
    std::vector<ParsedBlock>().swap(tl_blocks);
    std::vector<TxPart>().swap(tl_tx_parts);
}

}  // namespace host
}  // namespace bcc

using namespace bcc;
using namespace bcc::host;

namespace bcc {
namespace host {

int block_entry_txs(const bcc_tx_ref* items, size_t n, uint8_t* txid_out, uint8_t* wtxid_out,
                    int* err_out, int device, const BlockRulesCall* rules) {
    if (n == 0) return 0;
    if (!items) return -1;
    for (size_t i = 0; i < n; i++)
        if (!items[i].tx) return -1;
    reset_timing();
    BlockCounters c;
    const int rc = over_devices(device, std::vector<size_t>(n, 1), [&](int dev, size_t lo, size_t hi) {
        RangeState rs{dev, {}, c};
        return tx_range(items, lo, hi, txid_out, wtxid_out, err_out, rs, rules);
    });
    c.store();
    return rc ? -1 : 0;
}

int block_entry_blocks(const bcc_block_ref* blocks, size_t n, bcc_block_result* out, int device,
                       const BlockRulesCall* rules) {
    if (n == 0) return 0;
    if (!blocks || !out) return -1;
    for (size_t i = 0; i < n; i++)
        if (!blocks[i].block) return -1;
    reset_timing();
    std::vector<ParsedBlock>& parsed = tl_blocks;
    if (parsed.size() < n) parsed.resize(n);
    {
        ParseClock clock;
        pfor(n, 1, [&](size_t lo, size_t hi) {
            Tx tx;
            for (size_t b = lo; b < hi; b++) parse_block(blocks[b], parsed[b], tx, rules != nullptr);
        });
    }
    std::vector<size_t> weight(n);
    for (size_t b = 0; b < n; b++) weight[b] = parsed[b].jobs.size() + 1;
    BlockCounters c;
    const ParsedBlock* pb = parsed.data();
    const int rc = over_devices(device, weight, [&](int dev, size_t lo, size_t hi) {
        RangeState rs{dev, {}, c};
        return blocks_range(blocks, pb, lo, hi, out, rs, rules);
    });
    c.store();
    return rc ? -1 : 0;
}

}  // namespace host
}  // namespace bcc

extern "C" {

int bcc_tx_hashes_batch(const bcc_tx_ref* items, size_t n, unsigned char* txid_out,
                        unsigned char* wtxid_out, int* err_out, int device) {
    return block_entry_txs(items, n, txid_out, wtxid_out, err_out, device, nullptr);
}

int bcc_merkle_root(const unsigned char* leaves32, size_t n, unsigned char* root32, int* mutated,
                    int device) {
    if (!root32 || (n && !leaves32)) return -1;
    reset_timing();
    BlockCounters c;
    int rc = 0;
    uint32_t mut = 0;
    memset(root32, 0, 32);
    if (n >= BLOCK_MAX_BYTES / 32) {  // more leaves than the 32-bit records index
        ActiveCaller active;
        mut = merkle_root_host(leaves32, n, root32, true);
        c.t.round(n, 0, true);
    } else if (n) {
        ActiveCaller active;
        const MerkleSeg seg{0, (uint32_t)n, 0, 0};
        BlockRound r;
        r.leaves = leaves32;
        r.n_leaves = n;
        r.segs = &seg;
        r.n_segs = r.n_trees = 1;
        r.roots = root32;
        r.mut = &mut;
        RangeState rs{device < 0 ? device_list()[0] : device, {}, c};
        rc = run_round("merkle_root", r, n, n < BLOCK_MAX_BYTES / 32, rs);
        c.blocks++;
        c.txs += n;
        c.bytes += tree_bytes(n);
    }
    if (mutated) *mutated = mut != 0;
    c.store();
    return rc ? -1 : 0;
}

int bcc_block_commitments_batch(const bcc_block_ref* blocks, size_t n, bcc_block_result* out,
                                int device) {
    return block_entry_blocks(blocks, n, out, device, nullptr);
}

void bcc_last_block_stats(bcc_block_stats* out) {
    if (out) *out = t_block_stats;
}

int bcc_set_block_round(size_t txs) {
    g_block_round.store(txs, std::memory_order_relaxed);
    return 0;
}

int bcc_set_host_txhash_blocks(unsigned blocks) {
    g_host_txhash_blocks.store(blocks, std::memory_order_relaxed);
    return 0;
}

void bcc_block_last_timing_ms(double* ms6) {
    if (!ms6) return;
    for (int k = 0; k < BLOCK_MS_COUNT; k++) ms6[k] = 0;
    if (g_block_device_hook) g_block_device_hook->timing_ms(ms6, 0);
    ms6[BLOCK_MS_PARSE] = t_parse_ms;
}

}  // extern "C"
