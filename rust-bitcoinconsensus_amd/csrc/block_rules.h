// A block's transaction rules, sigops, finality, BIP34 height and sizes: the lane code the kernels
// (block_rules.hip), the host route (host/block_rules.cpp) and the stand-alone test program
// (tests/native/block_rules_host.cpp) all run, and what one round carries between them.  No HIP
// header here.
//
//   CheckTransaction (consensus/tx_check.cpp:10-58), GetLegacySigOpCount and IsFinalTx
//   (consensus/tx_verify.cpp:17-28, 107-119), CScript::GetSigOpCount(false) with GetScriptOp's
//   push rules (script/script.cpp:152-176, 281-331), and what CheckBlock / ContextualCheckBlock
//   sum and compare per block (validation.cpp:3387-3416, 3543-3620).
//
// A lane reads the transaction through a byte source (`u8(pos)`, `u32(pos)`): WordBytes over the
// round's 4-aligned raw blob (aligned dwords, bytes extracted by shifts; what the kernels use),
// PlainBytes over the caller's memory (the host route), or a checking one (the test program).
// Every position a lane reads lies in [base, base + len) of its transaction, whatever the bytes
// say: a walk that would leave it stops and marks the record TXR_MALFORMED.
#pragma once
#include <cstddef>
#include <cstdint>

#include "block_hash.h"

namespace bcc {

// ---- codes -------------------------------------------------------------------------------------
// The transaction codes are include/bcc_amd.h's BCC_TX_ERR_* (tx_check.cpp's reject strings in its
// order; 16 and up, clear of the deserialize errors the entries share with bcc_tx_hashes_batch).
enum : uint32_t {
    TXR_OK = 0,
    TXR_VIN_EMPTY = 16,
    TXR_VOUT_EMPTY = 17,
    TXR_OVERSIZE = 18,
    TXR_VOUT_NEGATIVE = 19,
    TXR_VOUT_TOOLARGE = 20,
    TXR_TXOUTTOTAL_TOOLARGE = 21,
    TXR_INPUTS_DUPLICATE = 22,
    TXR_CB_LENGTH = 23,
    TXR_PREVOUT_NULL = 24,
    TXR_MALFORMED = 255,  // the walk left the record's bytes: the host's parse and the lane disagree
};
constexpr int64_t BR_MAX_MONEY = 21000000ll * 100000000ll;
constexpr uint32_t BR_MAX_WEIGHT = 4000000, BR_WITNESS_SCALE = 4;
constexpr uint32_t BR_MAX_SIGOPS_COST = 80000;
constexpr uint32_t BR_LOCKTIME_THRESHOLD = 500000000;
constexpr uint32_t BR_NONE = 0xffffffffu;
enum : uint32_t { BR_SEGWIT_ACTIVE = 1, BR_BIP34_ACTIVE = 2 };  // bcc_block_check_ref::flags

// ---- byte sources ------------------------------------------------------------------------------
// Aligned dwords of a blob whose first byte is 4-aligned and which is readable up to the dword
// that holds the last byte read, plus one (the round's raw blob ends in four zero bytes).  The
// last dword read is kept: a script walk loads each dword once.
struct WordBytes {
    const uint32_t* w;
    uint32_t at = BR_NONE, cur = 0;
    SHA_HD explicit WordBytes(const uint32_t* words) : w(words) {}
    SHA_HD uint32_t word(uint32_t k) {
        if (k != at) {
            at = k;
            cur = w[k];
        }
        return cur;
    }
    SHA_HD uint32_t u8(uint32_t pos) { return (word(pos >> 2) >> (8 * (pos & 3))) & 0xff; }
    SHA_HD uint32_t u32(uint32_t pos) {
        const uint32_t s = 8 * (pos & 3), lo = word(pos >> 2);
        if (s == 0) return lo;
        return (lo >> s) | (word((pos >> 2) + 1) << (32 - s));
    }
};
struct PlainBytes {
    const uint8_t* p;
    SHA_HD explicit PlainBytes(const uint8_t* bytes) : p(bytes) {}
    SHA_HD uint32_t u8(uint32_t pos) { return p[pos]; }
    SHA_HD uint32_t u32(uint32_t pos) {
        return (uint32_t)p[pos] | (uint32_t)p[pos + 1] << 8 | (uint32_t)p[pos + 2] << 16 |
               (uint32_t)p[pos + 3] << 24;
    }
};

// ---- records -----------------------------------------------------------------------------------
// What tx_rules_lane leaves per transaction.  sig0 is tx-relative, so nothing here is
// round-relative.
struct TxRuleRec {
    uint32_t n_in, n_out;
    uint32_t stripped;    // bytes without marker, flag and witnesses
    uint32_t sigops;      // GetLegacySigOpCount
    uint32_t lock_time;
    uint32_t sig0_off, sig0_len;  // input 0's scriptSig inside the transaction (0, 0: no inputs)
    uint8_t is_coinbase, all_final;
    uint8_t before_dup;   // the first of vin-empty .. txouttotal-toolarge, or TXR_MALFORMED
    uint8_t after_dup;    // cb-length or prevout-null
    uint32_t dup;         // set by dup_input_lane (or the host's sort): two equal outpoints
};
static_assert(sizeof(TxRuleRec) == 36, "TxRuleRec: nine dwords");
SHA_HD uint32_t tx_rule_code(const TxRuleRec& r) {  // CheckTransaction's verdict
    return r.before_dup ? r.before_dup : r.dup ? (uint32_t)TXR_INPUTS_DUPLICATE : r.after_dup;
}

// One row of the input table: where the outpoint's 36 bytes start in the raw blob, and the
// transaction (the round's job index) it belongs to.
struct InRow {
    uint32_t off, tx;
};

// A block of the round: its transactions are jobs [job0, job0 + n_tx).
struct BlockRuleCtx {
    uint32_t job0, n_tx;
    int32_t height;
    uint32_t flags;        // BR_*
    int64_t cutoff;        // IsFinalTx's nBlockTime
    uint8_t bip34_len;     // the expected prefix CScript() << height, at most 6 bytes
    uint8_t bip34[7];
};
static_assert(sizeof(BlockRuleCtx) == 32, "BlockRuleCtx: two 16-byte loads");
struct BlockRuleBase {
    uint32_t job;  // the block's first job in the round
};
inline void rebase(BlockRuleCtx& c, const BlockRuleBase& b) { c.job0 += b.job; }

// What comes back per block.
struct BlockRuleOut {
    uint64_t sigops, stripped;  // sums over the block's transactions
    uint32_t cb_first;          // transaction 0 is a coinbase
    uint32_t cb_later;          // coinbases at positions >= 1
    uint32_t fail_tx, fail_code;  // the first transaction CheckTransaction refuses (BR_NONE: none)
    uint32_t nonfinal_tx;       // the first transaction IsFinalTx refuses (BR_NONE: none)
    uint32_t bip34_ok;
};
static_assert(sizeof(BlockRuleOut) == 40, "BlockRuleOut");

// The expected bytes of CScript() << height (script.h:432-445 push_int64, CScriptNum::serialize).
inline void bip34_prefix(int32_t height, uint8_t& len, uint8_t (&out)[7]) {
    for (uint8_t& b : out) b = 0;
    if (height == 0 || height == -1 || (height >= 1 && height <= 16)) {
        len = 1;
        out[0] = height == 0 ? 0x00 : (uint8_t)(height + 0x50);
        return;
    }
    const bool neg = height < 0;
    uint64_t a = neg ? (uint64_t)(-(int64_t)height) : (uint64_t)height;
    uint8_t n = 0;
    while (a) {
        out[1 + n++] = (uint8_t)(a & 0xff);
        a >>= 8;
    }
    if (out[n] & 0x80) out[1 + n++] = neg ? 0x80 : 0x00;
    else if (neg) out[n] |= 0x80;
    out[0] = n;
    len = (uint8_t)(n + 1);
}

// ---- the transaction lane ----------------------------------------------------------------------

// CScript::GetSigOpCount(false) over [pos, pos + n): a push that runs past the end stops the count.
template <class Bytes>
SHA_HD uint32_t script_sigops(Bytes& b, uint32_t pos, uint32_t n) {
    const uint32_t end = pos + n;
    uint32_t count = 0;
    while (pos < end) {
        const uint32_t op = b.u8(pos++);
        if (op <= 0x4e) {
            uint32_t size = op;
            if (op == 0x4c) {
                if (end - pos < 1) break;
                size = b.u8(pos);
                pos += 1;
            } else if (op == 0x4d) {
                if (end - pos < 2) break;
                size = b.u8(pos) | b.u8(pos + 1) << 8;
                pos += 2;
            } else if (op == 0x4e) {
                if (end - pos < 4) break;
                size = b.u32(pos);
                pos += 4;
            }
            if (end - pos < size) break;
            pos += size;
        } else if (op == 0xac || op == 0xad) {
            count += 1;
        } else if (op == 0xae || op == 0xaf) {
            count += 20;
        }
    }
    return count;
}

// The cursor of a walk over [pos, end): need(k) is asked before k bytes are read.
struct TxCursor {
    uint32_t pos, end;
    bool ok = true;
    SHA_HD bool need(uint32_t k) {
        if (!ok || end - pos < k) ok = false;
        return ok;
    }
};
// ReadCompactSize without the canonical check (the host's parse made it); values the vectors of a
// transaction cannot have (above MAX_SIZE) end the walk.
template <class Bytes>
SHA_HD uint32_t br_compact(Bytes& b, TxCursor& c) {
    if (!c.need(1)) return 0;
    const uint32_t f = b.u8(c.pos++);
    if (f < 253) return f;
    uint32_t v = 0;
    if (f == 253) {
        if (!c.need(2)) return 0;
        v = b.u8(c.pos) | b.u8(c.pos + 1) << 8;
        c.pos += 2;
    } else if (f == 254) {
        if (!c.need(4)) return 0;
        v = b.u32(c.pos);
        c.pos += 4;
    } else {
        if (!c.need(8)) return 0;
        v = b.u32(c.pos);
        if (b.u32(c.pos + 4)) c.ok = false;
        c.pos += 8;
    }
    if (v > 0x02000000u) c.ok = false;
    return c.ok ? v : 0;
}

// One transaction: `len` bytes at `base` of the source, its first witness byte at `wit` (0: the
// format without marker and flag), as the record of the hashing lane has them.  rows: when not
// null, the outpoint of input k < cap goes to rows[k] as (base + its offset, tx_row).
template <class Bytes>
SHA_HD TxRuleRec tx_rules_lane(Bytes& b, uint32_t base, uint32_t len, uint32_t wit, InRow* rows,
                               uint32_t cap, uint32_t tx_row) {
    TxRuleRec r{};
    r.stripped = wit ? wit - 2 + 4 : len;
    r.all_final = 1;
    if (len < 10 || (wit && (wit < 8 || wit > len - 4))) {
        r.before_dup = TXR_MALFORMED;
        return r;
    }
    // [version][marker flag] vin vout | witnesses | lock time
    TxCursor c{base + (wit ? 6u : 4u), base + (wit ? wit : len - 4)};
    const uint32_t n_in = br_compact(b, c);
    bool any_null = false, first_null = false;
    for (uint32_t k = 0; k < n_in && c.need(36); k++) {
        bool null = b.u32(c.pos + 32) == 0xffffffffu;
#pragma unroll
        for (int q = 0; q < 8; q++) null &= b.u32(c.pos + 4 * q) == 0;
        any_null |= null;
        if (k == 0) first_null = null;
        if (rows && k < cap) rows[k] = InRow{c.pos, tx_row};
        c.pos += 36;
        const uint32_t n = br_compact(b, c);
        if (!c.need(n + 4)) break;
        if (k == 0) {
            r.sig0_off = c.pos - base;
            r.sig0_len = n;
        }
        r.sigops += script_sigops(b, c.pos, n);
        c.pos += n;
        if (b.u32(c.pos) != 0xffffffffu) r.all_final = 0;
        c.pos += 4;
    }
    uint32_t n_out = 0;
    if (n_in == 0 && !wit) {  // no inputs: the flags byte follows, zero, and no output vector
        if (c.need(1) && b.u8(c.pos) != 0) c.ok = false;
        c.pos += 1;
    } else {
        n_out = br_compact(b, c);
    }
    uint32_t code = n_in == 0 ? (uint32_t)TXR_VIN_EMPTY
                    : n_out == 0 ? (uint32_t)TXR_VOUT_EMPTY
                    : (uint64_t)r.stripped * BR_WITNESS_SCALE > BR_MAX_WEIGHT ? (uint32_t)TXR_OVERSIZE
                                                                              : (uint32_t)TXR_OK;
    int64_t sum = 0;  // below 2 MAX_MONEY: every term and every partial sum is tested
    for (uint32_t k = 0; k < n_out && c.need(8); k++) {
        const int64_t v = (int64_t)((uint64_t)b.u32(c.pos) | (uint64_t)b.u32(c.pos + 4) << 32);
        c.pos += 8;
        if (code == TXR_OK) {
            if (v < 0) code = TXR_VOUT_NEGATIVE;
            else if (v > BR_MAX_MONEY) code = TXR_VOUT_TOOLARGE;
            else if ((sum += v) > BR_MAX_MONEY) code = TXR_TXOUTTOTAL_TOOLARGE;
        }
        const uint32_t n = br_compact(b, c);
        if (!c.need(n)) break;
        r.sigops += script_sigops(b, c.pos, n);
        c.pos += n;
    }
    if (!c.ok || c.pos != c.end) {
        r = TxRuleRec{};
        r.stripped = wit ? wit - 2 + 4 : len;
        r.before_dup = TXR_MALFORMED;
        return r;
    }
    r.n_in = n_in;
    r.n_out = n_out;
    r.lock_time = b.u32(base + len - 4);
    r.is_coinbase = n_in == 1 && first_null;
    r.before_dup = (uint8_t)code;
    if (r.is_coinbase) r.after_dup = r.sig0_len < 2 || r.sig0_len > 100 ? TXR_CB_LENGTH : TXR_OK;
    else r.after_dup = any_null ? TXR_PREVOUT_NULL : TXR_OK;
    return r;
}

// ---- the duplicate-input lane ------------------------------------------------------------------

// Slots of the table for `rows` input rows: a power of two, at least twice the rows, at least 2.
SHA_HD uint32_t dup_table_log2(uint64_t rows) {
    uint32_t l = 1;
    while (((uint64_t)1 << l) < 2 * rows) l++;
    return l;
}
// Where the key (transaction row, the outpoint's nine dwords) starts probing.
SHA_HD uint32_t outpoint_mix(uint32_t h, uint32_t w) {
    h = (h ^ w) * 0x9e3779b1u;
    return h ^ (h >> 15);
}
SHA_HD uint32_t outpoint_finish(uint32_t h, uint32_t log2_slots) {
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return h & (((uint32_t)1 << log2_slots) - 1);
}
template <class Bytes>
SHA_HD uint32_t outpoint_slot(Bytes& b, uint32_t tx_row, uint32_t off, uint32_t log2_slots) {
    uint32_t h = outpoint_mix(0x6f757470u, tx_row);
#pragma unroll
    for (int q = 0; q < 9; q++) h = outpoint_mix(h, b.u32(off + 4 * q));
    return outpoint_finish(h, log2_slots);
}
template <class Bytes>
SHA_HD bool outpoint_equal(Bytes& b, uint32_t x, uint32_t y) {
    bool same = true;
#pragma unroll
    for (int q = 0; q < 9; q++) same &= b.u32(x + 4 * q) == b.u32(y + 4 * q);
    return same;
}
// Input row `me`: claims the first free slot from its key's start (cas(slot, 0, me + 1) returns the
// word it found), and on the way compares itself with every occupant of its own transaction.
// Returns true when an equal outpoint sits in the table: the transaction has a duplicate.  The loop
// ends after one pass over the table whatever the words hold.
template <class Bytes, class Cas>
SHA_HD bool dup_input_lane(Bytes& b, const InRow* rows, uint32_t n_rows, uint32_t me, uint32_t* table,
                           uint32_t log2_slots, Cas cas) {
    const InRow mine = rows[me];
    const uint32_t mask = ((uint32_t)1 << log2_slots) - 1;
    uint32_t s = outpoint_slot(b, mine.tx, mine.off, log2_slots);
    for (uint32_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
        const uint32_t found = cas(table + s, 0u, me + 1);
        if (found == 0 || found == me + 1) return false;
        const uint32_t other = found - 1;
        if (other >= n_rows) continue;  // (not a word this round wrote)
        const InRow o = rows[other];
        if (o.tx == mine.tx && outpoint_equal(b, o.off, mine.off)) return true;
    }
    return false;
}

// ---- the block lane ----------------------------------------------------------------------------

SHA_HD bool tx_is_final(const TxRuleRec& r, int32_t height, int64_t cutoff) {
    if (r.lock_time == 0) return true;
    const int64_t lt = (int64_t)r.lock_time;
    if (lt < (lt < (int64_t)BR_LOCKTIME_THRESHOLD ? (int64_t)height : cutoff)) return true;
    return r.all_final != 0;
}

// What the transactions lo, lo + step, ... below n_tx of a block add up to; merge is associative
// and commutative, so any split of the block over lanes gives the same sums and minima.
struct BlockAcc {
    uint64_t sigops = 0, stripped = 0;
    uint64_t fail = ~(uint64_t)0;  // index << 8 | code of the first failing transaction
    uint32_t nonfinal = BR_NONE, cb_later = 0;
};
SHA_HD void block_acc_merge(BlockAcc& a, const BlockAcc& o) {
    a.sigops += o.sigops;
    a.stripped += o.stripped;
    a.fail = o.fail < a.fail ? o.fail : a.fail;
    a.nonfinal = o.nonfinal < a.nonfinal ? o.nonfinal : a.nonfinal;
    a.cb_later += o.cb_later;
}
SHA_HD BlockAcc block_rules_partial(const TxRuleRec* recs, const BlockRuleCtx& c, uint32_t lo,
                                    uint32_t step) {
    BlockAcc a;
    for (uint32_t k = lo; k < c.n_tx; k += step) {
        const TxRuleRec r = recs[(size_t)c.job0 + k];
        a.sigops += r.sigops;
        a.stripped += r.stripped;
        const uint32_t code = tx_rule_code(r);
        if (code && a.fail == ~(uint64_t)0) a.fail = (uint64_t)k << 8 | code;
        if (a.nonfinal == BR_NONE && !tx_is_final(r, c.height, c.cutoff)) a.nonfinal = k;
        if (k && r.is_coinbase) a.cb_later++;
    }
    return a;
}
// The block's result from the merged sums; tx0_base: where transaction 0 starts in the source.
template <class Bytes>
SHA_HD BlockRuleOut block_rules_finish(Bytes& b, const BlockAcc& a, const TxRuleRec& tx0,
                                       uint32_t tx0_base, const BlockRuleCtx& c) {
    BlockRuleOut o{};
    o.sigops = a.sigops;
    o.stripped = a.stripped;
    o.cb_first = tx0.is_coinbase;
    o.cb_later = a.cb_later;
    o.fail_tx = a.fail == ~(uint64_t)0 ? BR_NONE : (uint32_t)(a.fail >> 8);
    o.fail_code = a.fail == ~(uint64_t)0 ? 0u : (uint32_t)(a.fail & 0xff);
    o.nonfinal_tx = a.nonfinal;
    bool ok = tx0.before_dup != TXR_MALFORMED && tx0.sig0_len >= c.bip34_len && c.bip34_len <= 6;
    if (ok) {
        uint64_t want = 0;  // (shifted out below: no array is indexed by k)
#pragma unroll
        for (int q = 0; q < 7; q++) want |= (uint64_t)c.bip34[q] << (8 * q);
        for (uint32_t k = 0; k < c.bip34_len; k++)
            ok &= b.u8(tx0_base + tx0.sig0_off + k) == (uint32_t)((want >> (8 * k)) & 0xff);
    }
    o.bip34_ok = ok;
    return o;
}

// ---- one round's rules -------------------------------------------------------------------------
// Rides on a BlockRound (BlockRound::rules): the same jobs, the same upload.  in_base: n_jobs + 1
// prefix sums of the rows each job takes in the input table (its input count when that is two or
// more, from the host's parse); ctx: the round's blocks.  Results: one BlockRuleOut per block and,
// when `recs` is given (bcc_tx_check_batch), every job's record.
struct BlockRulesRound {
    const uint32_t* in_base = nullptr;
    const BlockRuleCtx* ctx = nullptr;
    size_t n_blocks = 0;
    BlockRuleOut* out = nullptr;
    TxRuleRec* recs = nullptr;
};
// what the device round requires of the records before any launch
inline bool block_rules_round_ok(const BlockRound& r, const BlockRulesRound& q) {
    if (!q.in_base || q.in_base[0] != 0) return false;
    for (size_t i = 0; i < r.n_jobs; i++)
        if (q.in_base[i + 1] < q.in_base[i]) return false;
    if (q.in_base[r.n_jobs] >= ((uint32_t)1 << 30)) return false;  // rows + 1 and 2 rows fit 32 bits
    for (size_t k = 0; k < q.n_blocks; k++) {
        const BlockRuleCtx& c = q.ctx[k];
        if (c.n_tx == 0 || c.job0 > r.n_jobs || c.n_tx > r.n_jobs - c.job0 || c.bip34_len > 6) return false;
    }
    return true;
}

// The device route of the rules (block_rules.hip): called by the block round with its arena.
// plan: the bytes it wants uploaded with the round's copy, page-locked and device-only; launch:
// after the round's upload and hashing launch are queued on `stream` (h_* / d_* its regions),
// queues its kernels and the copy of its results, and evaluates the long transactions on the host
// meanwhile; collect: after the stream was synchronised.
struct BlockRulesPlan {
    size_t up_bytes = 0, host_bytes = 0, dev_bytes = 0;
};
// event times of the three kernels, then host clocks: the plan and its records, the long transactions
enum { RULES_MS_TX = 0, RULES_MS_DUP, RULES_MS_BLOCK, RULES_MS_PLAN, RULES_MS_LONG, RULES_MS_COUNT };
struct BlockRulesDeviceHook {
    int (*plan)(const BlockRound& r, BlockRulesPlan& p);
    void (*fill)(const BlockRound& r, uint8_t* h_up);
    int (*launch)(const BlockRound& r, void* stream, const uint8_t* d_raw, const TxHashJob* d_jobs,
                  uint8_t* d_up, uint8_t* h_host, uint8_t* d_host, uint8_t* d_dev);
    void (*collect)(const BlockRound& r, const uint8_t* h_host);
    void (*timing_ms)(double* ms, int reset);
};
extern const BlockRulesDeviceHook* g_block_rules_device_hook;

namespace host {
// One job's record with the lane code over the caller's bytes, duplicates by a sort.
TxRuleRec tx_rules_job_host(const TxHashJob& j, const uint8_t* tx);
// The rules of a whole round on the host (r.rules), on the calling thread's team.
void block_rules_round_host(BlockRound& r);
}  // namespace host

}  // namespace bcc
