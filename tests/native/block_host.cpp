// tests/native/block_host.cpp — TEST ONLY.  Runs on the CPU what the block entries' device round
// runs (rust-bitcoinconsensus_amd/csrc/block_hash.h): the merkle lane code level by level over the
// level tables, exactly as block_hash.hip launches it, and the TxHashJob records of separate parts
// rebased into one round (pipeline.h BlockBase / rebase).  Links the engine's host code
// (engine_host.so) for the transaction parser and the host SHA-256.  Never linked into the product.
#include <cstring>
#include <vector>

#include "../../rust-bitcoinconsensus_amd/csrc/block_hash.h"
#include "../../rust-bitcoinconsensus_amd/csrc/host/tx.h"

using namespace bcc;

// bcc_merkle_root's contract over `trees` trees laid out back to back in leaves32 (n[t] leaves
// each): level 0 reads the leaves, later levels ping-pong between two buffers, one "launch" per
// level over every tree, the lanes run in descending order (no lane may depend on another).
// roots: 32 bytes per tree, mutated: one int per tree.  Returns the number of launches, -1 when
// the tables cannot be built.
extern "C" int block_host_merkle_lanes(const unsigned char* leaves32, const unsigned* n, unsigned trees,
                                       unsigned char* roots, int* mutated) {
    std::vector<MerkleSeg> segs;
    size_t rows = 0;
    for (unsigned t = 0; t < trees; t++) {
        segs.push_back(MerkleSeg{(uint32_t)rows, n[t], 0, t});
        rows += n[t];
    }
    std::vector<MerkleSeg> table;
    std::vector<uint32_t> level, lanes;
    if (!merkle_levels(segs.data(), segs.size(), table, level, lanes)) return -1;
    std::vector<uint32_t> nodes(8 * rows + 8), a(8 * rows + 8), b(8 * rows + 8), r(8 * trees + 8, 0),
        mut(trees + 1, 0);
    memcpy(nodes.data(), leaves32, 32 * rows);
    for (size_t k = 0; k < lanes.size(); k++) {
        const uint32_t* in = k == 0 ? nodes.data() : (k & 1 ? a.data() : b.data());
        uint32_t* out = k & 1 ? b.data() : a.data();
        for (uint32_t g = lanes[k]; g-- > 0;) {
            const MerkleLane L = merkle_lane(table.data() + level[k], level[k + 1] - level[k], g, in,
                                             out, r.data());
            if (merkle_lane_run(L)) mut[L.seg] |= 1u;
        }
    }
    memcpy(roots, r.data(), 32 * (size_t)trees);
    for (unsigned t = 0; t < trees; t++) mutated[t] = (int)mut[t];
    return (int)lanes.size();
}

// Transactions tx[0 .. n) (lengths len[i], all of them parse) in parts cut at part[0] = 0 < ... <
// part[P] = n.  Every part builds its records from zero (offsets into its own blob, rows from 0)
// and is hashed alone into alone_*; then the parts' blobs are concatenated, the records rebased
// with each part's BlockBase, checked with txh_job_ok against the merged blob and hashed from it
// into merged_*.  wtxid rows are wanted for every transaction.  Returns 0, or 1 + the index of
// the first record that fails a check.
extern "C" int block_host_rebase(const unsigned char* const* tx, const unsigned* len, unsigned n,
                                 const unsigned* part, unsigned P, unsigned char* alone_txid,
                                 unsigned char* alone_wtxid, unsigned char* merged_txid,
                                 unsigned char* merged_wtxid) {
    std::vector<uint8_t> merged;
    std::vector<TxHashJob> all(n);
    host::Tx t;
    for (unsigned p = 0; p < P; p++) {
        std::vector<uint8_t> blob;
        std::vector<TxHashJob> jobs;
        for (unsigned i = part[p]; i < part[p + 1]; i++) {
            if (!host::parse_tx(tx[i], len[i], t) || t.ser_size != len[i]) return 1 + (int)i;
            TxHashJob j{};
            j.off = (uint32_t)blob.size();
            j.len = len[i];
            if (t.has_witness())
                j.wit = (uint32_t)((t.vout.empty() ? t.vin.back().script_sig.end() + 5
                                                   : t.vout.back().ser.end()) - tx[i]);
            j.row = i - part[p];
            j.flags = TXH_W;
            jobs.push_back(j);
            blob.insert(blob.end(), tx[i], tx[i] + len[i]);
        }
        const size_t m = jobs.size();
        std::vector<uint8_t> tr(32 * m + 1), wr(32 * m + 1);
        for (size_t k = 0; k < m; k++) {
            if (!txh_job_ok(jobs[k], blob.size(), m)) return 1 + (int)(part[p] + k);
            host::tx_hash_job_host(jobs[k], blob.data() + jobs[k].off, tr.data(), wr.data());
        }
        memcpy(alone_txid + 32 * (size_t)part[p], tr.data(), 32 * m);
        memcpy(alone_wtxid + 32 * (size_t)part[p], wr.data(), 32 * m);
        if (m) rebase_copy(&all[part[p]], jobs.data(), m, BlockBase{(uint32_t)merged.size(), part[p]});
        merged.insert(merged.end(), blob.begin(), blob.end());
    }
    for (unsigned i = 0; i < n; i++) {
        if (!txh_job_ok(all[i], merged.size(), n) || all[i].row != i) return 1 + (int)i;
        host::tx_hash_job_host(all[i], merged.data() + all[i].off, merged_txid, merged_wtxid);
    }
    return 0;
}

// the chain length the long-chain threshold is compared with, for a record of these fields
extern "C" unsigned block_host_chain_blocks(unsigned len, unsigned wit, unsigned flags) {
    TxHashJob j{};
    j.len = len;
    j.wit = wit;
    j.flags = flags;
    return txh_chain_blocks(j);
}
