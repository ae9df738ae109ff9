// The block entries' round machinery (block.cpp: the parsers, the round cuts, the failure rules,
// the device shares) as the rule entries (block_rules.cpp) drive it: the same rounds over the same
// upload, with the rules riding along (BlockRound::rules).
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>

#include "../block_rules.h"
#include "bcc_amd.h"

namespace bcc {
namespace host {

// The callbacks run on whichever thread drives a device share, for disjoint blocks or items.
struct BlockRulesCall {
    // block b's context: height, flags, cutoff and the BIP34 prefix (job0 and n_tx are the round's)
    std::function<BlockRuleCtx(size_t b)> ctx;
    // block b's commitment result and, when it has transactions, what its lanes found
    std::function<void(size_t b, const bcc_block_result& commit, const BlockRuleOut* rules)> block;
    // item i: its parse error, or its record
    std::function<void(size_t i, int err, const TxRuleRec* rec)> tx;
};

// bcc_block_commitments_batch, bcc_tx_hashes_batch (rules == nullptr) and the rule entries.
int block_entry_blocks(const bcc_block_ref* blocks, size_t n, bcc_block_result* out, int device,
                       const BlockRulesCall* rules);
int block_entry_txs(const bcc_tx_ref* items, size_t n, uint8_t* txid_out, uint8_t* wtxid_out,
                    int* err_out, int device, const BlockRulesCall* rules);

}  // namespace host
}  // namespace bcc
