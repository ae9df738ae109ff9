// A block's transaction rules, sigops, finality, coinbase height and sizes: bcc_tx_check_batch and
// bcc_block_check_batch (include/bcc_amd.h).
//
// Host half: the entries ride on the block entries' rounds (block_entry.h): block.cpp parses, cuts
// the rounds and runs them under the failure rules, and a round carries a BlockRulesRound beside its
// hashing jobs.  Here: the context records (height, cutoff, the expected BIP34 prefix), the host
// evaluation of a round's rules with the lane code of block_rules.h (small rounds, rounds the
// device could not deliver, the long transactions of a device round), and the merge of a block's
// commitment result with its rule record in Core's order.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../block_rules.h"
#include "bcc_amd.h"
#include "block_entry.h"
#include "team.h"
#include "tuples.h"

namespace bcc {

const BlockRulesDeviceHook* g_block_rules_device_hook = nullptr;

namespace host {

// One job on the host: the lane over the caller's bytes, its outpoints sorted for the duplicate check.
TxRuleRec tx_rules_job_host(const TxHashJob& j, const uint8_t* tx) {
    thread_local std::vector<InRow> rows;
    rows.resize(j.len / 41 + 1);  // (an input takes 41 bytes or more)
    PlainBytes b(tx);
    TxRuleRec r = tx_rules_lane(b, 0, j.len, j.wit, rows.data(), (uint32_t)rows.size(), 0);
    if (r.before_dup == TXR_MALFORMED || r.n_in < 2) return r;
    std::sort(rows.begin(), rows.begin() + r.n_in,
              [&](const InRow& x, const InRow& y) { return memcmp(tx + x.off, tx + y.off, 36) < 0; });
    for (uint32_t k = 0; k + 1 < r.n_in; k++)
        if (memcmp(tx + rows[k].off, tx + rows[k + 1].off, 36) == 0) r.dup = 1;
    return r;
}

void block_rules_round_host(BlockRound& r) {
    BlockRulesRound& q = *r.rules;
    thread_local std::vector<TxRuleRec> own;
    TxRuleRec* recs = q.recs;
    if (!recs) {
        own.resize(r.n_jobs);
        recs = own.data();
    }
    pfor(r.n_jobs, 64, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) recs[i] = tx_rules_job_host(r.jobs[i], r.src[i]);
    });
    pfor(q.n_blocks, 1, [&](size_t lo, size_t hi) {
        for (size_t k = lo; k < hi; k++) {
            const BlockRuleCtx& c = q.ctx[k];
            const BlockAcc a = block_rules_partial(recs, c, 0, 1);
            PlainBytes b(r.src[c.job0]);
            q.out[k] = block_rules_finish(b, a, recs[c.job0], 0, c);
        }
    });
}

namespace {

size_t compact_size_len(uint64_t v) { return v < 253 ? 1 : v <= 0xffff ? 3 : v <= 0xffffffffull ? 5 : 9; }

// Core's order over what the commitments round and the rule lanes found.
void merge_block(const bcc_block_check_ref& ref, const bcc_block_result& c, const BlockRuleOut* o,
                 bcc_block_check_result& R) {
    memset(&R, 0, sizeof R);
    R.status = c.status;
    R.tx_index = -1;
    R.n_tx = c.n_tx;
    R.commit_pos = c.commit_pos;
    memcpy(R.merkle_root, c.merkle_root, 32);
    memcpy(R.witness_root, c.witness_root, 32);
    if (!o) return;  // it did not deserialize, or is empty
    R.sigops = o->sigops;
    R.stripped_size = 80 + compact_size_len(c.n_tx) + o->stripped;
    R.weight = 3 * R.stripped_size + ref.block_len;
    if (o->fail_tx != BR_NONE && o->fail_code == TXR_MALFORMED) {  // (the lanes and the parser disagree)
        R.status = BCC_BLOCK_ERR_DESERIALIZE;
        return;
    }
    if (c.status == BCC_BLOCK_ERR_MERKLE_ROOT || c.status == BCC_BLOCK_ERR_DUPLICATE) return;
    if ((uint64_t)c.n_tx * BR_WITNESS_SCALE > BR_MAX_WEIGHT ||
        R.stripped_size * BR_WITNESS_SCALE > BR_MAX_WEIGHT) {
        R.status = BCC_BLOCK_ERR_LENGTH;
    } else if (!o->cb_first) {
        R.status = BCC_BLOCK_ERR_CB_MISSING;
    } else if (o->cb_later) {
        R.status = BCC_BLOCK_ERR_CB_MULTIPLE;
    } else if (o->fail_tx != BR_NONE) {
        R.status = BCC_BLOCK_ERR_TX;
        R.tx_index = (int)o->fail_tx;
        R.tx_status = (int)o->fail_code;
    } else if (o->sigops * BR_WITNESS_SCALE > BR_MAX_SIGOPS_COST) {
        R.status = BCC_BLOCK_ERR_SIGOPS;
    } else if (o->nonfinal_tx != BR_NONE) {
        R.status = BCC_BLOCK_ERR_NONFINAL;
        R.tx_index = (int)o->nonfinal_tx;
    } else if ((ref.flags & BCC_BLOCK_BIP34_ACTIVE) && !o->bip34_ok) {
        R.status = BCC_BLOCK_ERR_CB_HEIGHT;
    } else if (c.status) {  // the witness commitment
        R.status = c.status;
    } else if (R.weight > BR_MAX_WEIGHT) {
        R.status = BCC_BLOCK_ERR_WEIGHT;
    }
}

}  // namespace
}  // namespace host
}  // namespace bcc

using namespace bcc;
using namespace bcc::host;

extern "C" {

int bcc_tx_check_batch(const bcc_tx_ref* items, size_t n, bcc_tx_check_result* out, int device) {
    if (n == 0) return 0;
    if (!items || !out) return -1;
    BlockRulesCall call;
    call.tx = [&](size_t i, int err, const TxRuleRec* r) {
        bcc_tx_check_result& R = out[i];
        memset(&R, 0, sizeof R);
        R.status = err;
        if (!r) return;
        const uint32_t code = tx_rule_code(*r);
        R.status = code == TXR_MALFORMED ? (int)bitcoinconsensus_ERR_TX_DESERIALIZE : (int)code;
        if (code == TXR_MALFORMED) return;
        R.n_in = r->n_in;
        R.n_out = r->n_out;
        R.sigops = r->sigops;
        R.lock_time = r->lock_time;
        R.stripped_size = r->stripped;
        R.total_size = items[i].tx_len;
        R.is_coinbase = r->is_coinbase;
        R.all_final = r->all_final;
    };
    return block_entry_txs(items, n, nullptr, nullptr, nullptr, device, &call);
}

int bcc_block_check_batch(const bcc_block_check_ref* blocks, size_t n, bcc_block_check_result* out,
                          int device) {
    if (n == 0) return 0;
    if (!blocks || !out) return -1;
    std::vector<bcc_block_ref> refs(n);
    for (size_t b = 0; b < n; b++) {
        if (!blocks[b].block) return -1;
        refs[b] = bcc_block_ref{blocks[b].block, blocks[b].block_len,
                                (blocks[b].flags & BCC_BLOCK_SEGWIT_ACTIVE) ? 1 : 0, nullptr, 0};
    }
    std::vector<bcc_block_result> commit(n);
    BlockRulesCall call;
    call.ctx = [&](size_t b) {
        BlockRuleCtx c{};
        c.height = blocks[b].height;
        c.flags = blocks[b].flags;
        c.cutoff = blocks[b].lock_time_cutoff;
        bip34_prefix(c.height, c.bip34_len, c.bip34);
        return c;
    };
    call.block = [&](size_t b, const bcc_block_result& c, const BlockRuleOut* o) {
        merge_block(blocks[b], c, o, out[b]);
    };
    return block_entry_blocks(refs.data(), n, commit.data(), device, &call);
}

void bcc_block_rules_last_timing_ms(double* ms5) {
    if (!ms5) return;
    for (int k = 0; k < RULES_MS_COUNT; k++) ms5[k] = 0;
    if (g_block_rules_device_hook) g_block_rules_device_hook->timing_ms(ms5, 0);
}

unsigned int bcc_debug_outpoint_slot(unsigned int tx_row, const unsigned char* outpoint36,
                                     unsigned int log2_slots) {
    if (!outpoint36 || log2_slots < 1 || log2_slots > 31) return 0;
    PlainBytes b(outpoint36);
    return outpoint_slot(b, tx_row, 0, log2_slots);
}

unsigned int bcc_debug_dup_table_log2(size_t rows) { return dup_table_log2(rows); }

}  // extern "C"
