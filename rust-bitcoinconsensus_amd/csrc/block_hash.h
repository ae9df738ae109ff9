// Transaction hashes and merkle trees of whole blocks: what one round carries between the host
// pass (host/block.cpp) and the device (block_hash.hip), the merkle lane both run, and the level
// tables.  No HIP header here: csrc/host and the CPU test builds include this.
//
//   txid  = SHA-256d of the serialization without marker, flag and witnesses
//   wtxid = SHA-256d of every byte (primitives/transaction.cpp:67-83)
//   ComputeMerkleRoot (consensus/merkle.cpp:45-62): level by level SHA-256d(left || right), an odd
//   level's last node paired with itself, `mutated` when two existing siblings are equal.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "pipeline.h"
#include "sha256_device.h"

namespace bcc {

// 64-byte blocks of the SHA-256 chain over len message bytes (0x80, 8 length bytes)
inline uint32_t sha_chain_blocks(uint32_t len) { return (uint32_t)(((uint64_t)len + 9 + 63) / 64); }
// bytes of a job's txid message
inline uint32_t txh_stripped_len(const TxHashJob& j) { return j.wit ? j.wit - 2 + 4 : j.len; }
// whether the job takes a wtxid lane of its own (else the wtxid row, if wanted, is a copy or zero)
inline bool txh_w_lane(const TxHashJob& j) { return j.wit && (j.flags & (TXH_W | TXH_WZERO)) == TXH_W; }
// the longest chain among the job's lanes
inline uint32_t txh_chain_blocks(const TxHashJob& j) {
    return sha_chain_blocks(txh_w_lane(j) ? j.len : txh_stripped_len(j));
}
// what the kernel requires of a record before it reads a byte
inline bool txh_job_ok(const TxHashJob& j, size_t raw_bytes, size_t rows) {
    if (j.len < 10 || j.off > raw_bytes || j.len > raw_bytes - j.off || j.row >= rows) return false;
    return j.wit == 0 || (j.wit >= 6 + 1 + 1 && j.wit <= j.len - 4);
}

// One tree of a level: n_in nodes at rows [base, base + n_in) of the level's input, lanes
// [lane0, lane0 + merkle_seg_lanes) of the launch, results for tree `seg`.  n_in == 1 happens
// on level 0 only (a single leaf is its own root: one lane copies it); a tree whose level has one
// parent writes it to the roots and leaves the table.
struct MerkleSeg {
    uint32_t base, n_in, lane0, seg;
};
inline uint32_t merkle_seg_lanes(uint32_t n_in) { return n_in == 1 ? 1u : (n_in + 1) / 2; }

// The tables of every level from level 0's trees (lane0 ignored on input; trees with n_in == 0
// take no part: their root is the caller's).  level[k] .. level[k + 1] index `table`, lanes[k] is
// level k's launch size.  False when a level would not fit 32-bit lane numbers.
inline bool merkle_levels(const MerkleSeg* segs0, size_t n, std::vector<MerkleSeg>& table,
                          std::vector<uint32_t>& level, std::vector<uint32_t>& lanes) {
    table.clear();
    level.assign(1, 0);
    lanes.clear();
    std::vector<MerkleSeg> cur;
    for (size_t s = 0; s < n; s++)
        if (segs0[s].n_in) cur.push_back(segs0[s]);
    while (!cur.empty()) {
        uint64_t l = 0;
        std::vector<MerkleSeg> next;
        for (MerkleSeg& m : cur) {
            m.lane0 = (uint32_t)l;
            l += merkle_seg_lanes(m.n_in);
            if (l >= ((uint64_t)1 << 31)) return false;
            table.push_back(m);
            if (m.n_in > 2) next.push_back(MerkleSeg{m.base, (m.n_in + 1) / 2, 0, m.seg});
        }
        level.push_back((uint32_t)table.size());
        lanes.push_back((uint32_t)l);
        cur.swap(next);
    }
    return true;
}

// SHA-256d of the 64 bytes l || r, all as big-endian words: the message block, the constant
// padding block of a 64-byte message, then the digest's own block.
SHA_HD void merkle_node(uint32_t (&out)[8], const uint32_t (&l)[8], const uint32_t (&r)[8]) {
    uint32_t s[8], w[16];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        w[j] = l[j];
        w[8 + j] = r[j];
    }
    sha256_init_state(s);
    sha256_compress(s, w);
    w[0] = 0x80000000u;
#pragma unroll
    for (int j = 1; j < 15; j++) w[j] = 0;
    w[15] = 64 * 8;
    sha256_compress(s, w);
    sha256_of_digest(out, s);
}

// Lane g of one level (tab: the level's n_tab >= 1 trees, g below the level's lane count): where
// it reads and writes.  Rows are 32 bytes, as raw digest bytes.
struct MerkleLane {
    const uint32_t *l, *r;  // r == l: the self-paired last node of an odd level, or a copy
    uint32_t* out;
    uint32_t seg;
    bool copy;  // n_in == 1: out = l, nothing is hashed
    bool pair;  // both children exist: equal children set the tree's mutation word
};
SHA_HD MerkleLane merkle_lane(const MerkleSeg* tab, uint32_t n_tab, uint32_t g, const uint32_t* in,
                              uint32_t* out, uint32_t* roots) {
    uint32_t lo = 0, hi = n_tab;  // the last tree with lane0 <= g
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (tab[mid].lane0 <= g) lo = mid;
        else hi = mid;
    }
    const MerkleSeg m = tab[lo];
    const uint32_t k = g - m.lane0;
    MerkleLane L;
    L.seg = m.seg;
    L.copy = m.n_in == 1;
    L.pair = 2 * k + 1 < m.n_in;
    L.l = in + 8 * ((size_t)m.base + 2 * k);
    L.r = L.pair ? L.l + 8 : L.l;
    L.out = m.n_in <= 2 ? roots + 8 * (size_t)m.seg : out + 8 * ((size_t)m.base + k);
    return L;
}
SHA_HD uint32_t merkle_bswap(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bswap32(x);
#else
    return sha_bswap(x);
#endif
}
// The lane's work but for the mutation word: returns whether the tree's word is to be set.
SHA_HD bool merkle_lane_run(const MerkleLane& L) {
    uint32_t a[8], b[8], d[8];
    bool same = true;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        a[j] = L.l[j];
        b[j] = L.r[j];
        same &= a[j] == b[j];
    }
    if (L.copy) {
#pragma unroll
        for (int j = 0; j < 8; j++) L.out[j] = a[j];
        return false;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        a[j] = merkle_bswap(a[j]);
        b[j] = merkle_bswap(b[j]);
    }
    merkle_node(d, a, b);
#pragma unroll
    for (int j = 0; j < 8; j++) L.out[j] = merkle_bswap(d[j]);
    return L.pair && same;
}

// One round.  Transactions: job i's bytes are at src[i] in the caller's memory and at jobs[i].off
// in the raw blob (raw_bytes long; the device route copies them there).  Node rows: the txid rows
// [0, rows), then the wtxid rows [rows, 2 rows); or, with `leaves`, the n_leaves given rows
// (bcc_merkle_root: no jobs).  A row no job names comes back as zeros (bcc_tx_hashes_batch: an
// item that does not parse); rounds with trees have a job for every row.  segs: level 0's trees
// over the node rows, each with the index of its root row and mutation word (the rows of trees no
// seg names keep what the caller wrote).
struct BlockRulesRound;  // block_rules.h
struct BlockRound {
    const TxHashJob* jobs = nullptr;
    const uint8_t* const* src = nullptr;
    size_t n_jobs = 0, rows = 0, raw_bytes = 0;
    unsigned host_blocks = 0;  // jobs whose chain is longer go to the host (0: none)
    const uint8_t* leaves = nullptr;
    size_t n_leaves = 0;
    const MerkleSeg* segs = nullptr;
    size_t n_segs = 0;
    size_t n_trees = 0;  // rows of `roots` and words of `mut`: every segs[s].seg is below it
    // results: 32 bytes per row (txid is required with jobs, wtxid may be null), 32 bytes and one
    // word per tree
    uint8_t* txid = nullptr;
    uint8_t* wtxid = nullptr;
    uint8_t* roots = nullptr;
    uint32_t* mut = nullptr;
    // the transaction and block rules over the same jobs (block_rules.h); null: hashes only
    BlockRulesRound* rules = nullptr;
    // counted by whoever runs the round
    size_t long_txs = 0, merkle_launches = 0;
    size_t node_rows() const { return leaves ? n_leaves : 2 * rows; }
};

// The device route, set by block_hash.hip when the library loads; null in a build without the
// kernels (the CPU tests' engine), where a device round is the host evaluation.
// round: 0 or the HIP error; timing_ms: the calling thread's times since reset (BLOCK_MS_TXH ..
// BLOCK_MS_STAGE; the event times are zero without BCC_BLOCK_TIMING=1 in the environment).
enum { BLOCK_MS_TXH = 0, BLOCK_MS_MERKLE, BLOCK_MS_UPLOAD, BLOCK_MS_DOWNLOAD, BLOCK_MS_PARSE,
       BLOCK_MS_STAGE, BLOCK_MS_COUNT };
struct BlockDeviceHook {
    int (*round)(int device, BlockRound& r);
    void (*timing_ms)(double* ms, int reset);  // ms may be null; BLOCK_MS_PARSE is not its own
};
extern const BlockDeviceHook* g_block_device_hook;

namespace host {
// One job's digests with host SHA-256 (what a lane pair of K_txh writes): the txid row and, per
// the job's flags, the wtxid row.
void tx_hash_job_host(const TxHashJob& j, const uint8_t* tx, uint8_t* txid_rows, uint8_t* wtxid_rows);
// The whole round on the host, on up to `threads` team threads.
void block_round_host(BlockRound& r, unsigned threads);
// ComputeMerkleRoot over n 32-byte leaves (n >= 1); returns the mutation flag.  team: the levels
// are split over the calling thread's team (not from a team thread).
bool merkle_root_host(const uint8_t* leaves, size_t n, uint8_t* root32, bool team);
}  // namespace host

}  // namespace bcc
