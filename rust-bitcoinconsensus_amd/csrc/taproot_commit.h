// BIP341 script-path commitment, per lane (one lane = one spend) and the host row builder.
//
// Restates VerifyTaprootCommitment (script/interpreter.cpp:1834-1853) and
// XOnlyPubKey::CheckPayToContract (pubkey.cpp:184-189) =
// secp256k1_xonly_pubkey_parse + secp256k1_xonly_pubkey_tweak_add_check
// (secp256k1/src/modules/extrakeys/main_impl.h:21-41, 109-129):
//   k = TapLeaf(leaf_version || compact_size(len) || script)
//   k = TapBranch(min(k, node) || max(k, node))        per 32-byte node of the control block
//   t = TapTweak(p || k)
//   lift_x(p) + t G == (q, parity)
// The hashing half (commit_hash_lane) is SHA-bound with a per-lane trip count; the curve half
// (tweak_add_lane + tweak_fin_lane) has no variable-base ladder: one square root for lift_x, the
// fixed-base comb of ecdsa_twist.h for t G, one mixed addition with its doubling / infinity cases,
// and an inversion that the kernels batch over a group of lanes (taproot_commit.hip).
// Everything is BCC_HD, so the CPU tests run the kernels' exact arithmetic.
#pragma once
#include <cstring>

#include "bcc_amd.h"
#include "ecdsa_twist.h"

namespace bcc {

// ------------------------------------------------------------------------------------------
// hashing half
// ------------------------------------------------------------------------------------------

// SHA-256 states after the 64-byte prefix SHA256(tag) || SHA256(tag) of the three tagged hashes
// (CHashWriter TaggedHash, hash.cpp:89-96)
struct CommitMids {
    u32 leaf[8], branch[8], tweak[8];
};

inline void tagged_midstate(u32 out[8], const char* tag) {
    const size_t len = strlen(tag);  // < 56: one padded block
    uint8_t b[64] = {0};
    memcpy(b, tag, len);
    b[len] = 0x80;
    b[62] = (uint8_t)((len * 8) >> 8);
    b[63] = (uint8_t)(len * 8);
    u32 w[16], d[8];
    for (int j = 0; j < 16; j++)
        w[j] = ((u32)b[4 * j] << 24) | ((u32)b[4 * j + 1] << 16) | ((u32)b[4 * j + 2] << 8) | b[4 * j + 3];
    sha256_init_state(d);
    sha256_compress(d, w);
    for (int j = 0; j < 8; j++) w[j] = w[8 + j] = d[j];
    sha256_init_state(out);
    sha256_compress(out, w);
}

inline CommitMids commit_mids() {
    CommitMids m;
    tagged_midstate(m.leaf, "TapLeaf");
    tagged_midstate(m.branch, "TapBranch");
    tagged_midstate(m.tweak, "TapTweak");
    return m;
}

// out = tagged hash of the 64-byte message a || b from the tag midstate: two compressions (the
// message block, then the padding block of a 128-byte total).  Words are big-endian (word 0 =
// bytes 0-3).  out may alias a or b.
BCC_HD void tagged64_lane(u32 (&out)[8], const u32 (&a)[8], const u32 (&b)[8], const u32* mid) {
    u32 s[8], w[16];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        s[j] = mid[j];
        w[j] = a[j];
        w[8 + j] = b[j];
    }
    sha256_compress(s, w);
    w[0] = 0x80000000u;
#pragma unroll
    for (int j = 1; j < 15; j++) w[j] = 0;
    w[15] = 128 * 8;
    sha256_compress(s, w);
#pragma unroll
    for (int j = 0; j < 8; j++) out[j] = s[j];
}

// k = TapBranch(min(k, node) || max(k, node)) by bytewise lexicographic order
// (interpreter.cpp:1843-1849: std::lexicographical_compare(k, node) puts k first only when it is
// strictly smaller, so an equal node goes first).  On big-endian words that order is the order
// of the first differing word.
BCC_HD void tapbranch_lane(u32 (&k)[8], const u32 (&node)[8], const u32* mid) {
    bool k_less = false;
#pragma unroll
    for (int j = 7; j >= 0; j--)  // the most significant differing word decides (written last)
        if (k[j] != node[j]) k_less = k[j] < node[j];
    u32 a[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        a[j] = k_less ? k[j] : node[j];
        b[j] = k_less ? node[j] : k[j];
    }
    tagged64_lane(k, a, b, mid);
}

// 32 bytes at p (4-byte aligned) as big-endian words
BCC_HD void load_be_words(u32 (&w)[8], const u32* p) {
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = bswap32(p[j]);
}
BCC_HD void store_be_words(u32* p, const u32 (&w)[8]) {
#pragma unroll
    for (int j = 0; j < 8; j++) p[j] = bswap32(w[j]);
}

// The hashing half of one spend.  leaf_blocks = the nblk 64-byte blocks of the padded leaf message
// (commit_fill_leaf: the padding counts the 64-byte tag prefix), nodes = depth 32-byte nodes,
// p_raw = the internal key's 32 bytes; all 4-byte aligned.  leaf and t as big-endian words.
BCC_HD void commit_hash_lane(const CommitMids& m, const u32* leaf_blocks, u32 nblk, const u32* nodes,
                             u32 depth, const u32* p_raw, u32 (&leaf)[8], u32 (&t)[8]) {
    u32 k[8];
#pragma unroll
    for (int j = 0; j < 8; j++) k[j] = m.leaf[j];
#pragma unroll 1
    for (u32 b = 0; b < nblk; b++) {
        u32 w[16];
#pragma unroll
        for (int j = 0; j < 16; j++) w[j] = bswap32(leaf_blocks[16 * (size_t)b + j]);
        sha256_compress(k, w);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) leaf[j] = k[j];
#pragma unroll 1
    for (u32 d = 0; d < depth; d++) {
        u32 node[8];
        load_be_words(node, nodes + 8 * (size_t)d);
        tapbranch_lane(k, node, m.branch);
    }
    u32 p[8];
    load_be_words(p, p_raw);
    tagged64_lane(t, p, k, m.tweak);
}

// ------------------------------------------------------------------------------------------
// curve half
// ------------------------------------------------------------------------------------------

// what tweak_add_lane decided: the verdict itself, or "R is a finite point: compare it"
enum : u32 { TC_FALSE = 0, TC_TRUE = 1, TC_NORMAL = 2 };

// the comb's view of a scalar (the slots of TwistState it reads)
struct CombScalar {
    u32 k[4][4];
    u32 flags;
    BCC_HD u32 kword(int s, int w) const { return k[s][w]; }
};

// R = lift_x(p) + t G (Jacobian) for the canonical-or-not 32-byte values p, q, t as read from
// their big-endian strings.  Decides every row that needs no comparison of R:
//   parity byte not 0 / 1, t >= n (scalar_set_b32 overflow), p >= the field prime or p^3 + 7 not a
//   square (xonly_pubkey_parse), q >= the field prime (its 32 bytes can never equal a serialized
//   x), R = infinity                                                          -> TC_FALSE
//   t = 0: R = lift_x(p) itself, even y                                       -> q == p && parity == 0
template <class GC>
BCC_HD u32 tweak_add_lane(const fe& p, const fe& q, u32 parity, const sc& t, const GC& gc, gej& R) {
    const u32 N[8] = BCC_N_LIMBS;
    if (parity > 1u || !u256_lt(t.v, N) || !fe_lt_p(p) || !fe_lt_p(q)) return TC_FALSE;
    fe v, y;
    curve_rhs(v, p);
    if (!fe_sqrt(y, v)) return TC_FALSE;
    fe_normalize(y);
    if (y.v[0] & 1u) {  // the even-y lift (ge_set_xo_var(.., 0)); y != 0: the curve has no 2-torsion
        fe_neg(y, y);
        fe_normalize(y);
    }
    CombScalar cs;
    cs.flags = LS_VALID;
    sc u = t;
    if (sc_is_zero(u)) {
        cs.flags |= LS_U1ZERO;
        u.v[0] = 1u;
    } else if ((u.v[0] & 1u) == 0) {  // the comb wants an odd scalar: t G = -((n - t) G)
        sc_neg(u, u);
        cs.flags |= LS_NEGU1;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        cs.k[0][i] = cs.k[1][i] = 0;
        cs.k[2][i] = u.v[i];
        cs.k[3][i] = u.v[4 + i];
    }
    gej A;
    if (twist_accumulate_g(cs, gc, A)) {  // t G is the point at infinity: t = 0
        bool same = true;
#pragma unroll
        for (int i = 0; i < 8; i++) same &= p.v[i] == q.v[i];
        return same && parity == 0 ? TC_TRUE : TC_FALSE;
    }
    bool inf;
    gej_add_zinv(R, inf, A, p, y, fe_one(), false);  // doubles when t G == lift_x(p)
    return inf ? TC_FALSE : TC_NORMAL;
}

// The comparison for a TC_NORMAL row: zinv = R.z^-1; q is canonical (tweak_add_lane checked).
BCC_HD int tweak_fin_lane(const gej& R, const fe& zinv, const fe& q, u32 parity) {
    fe z2, z3, x, y;
    fe_sqr(z2, zinv);
    fe_mul(z3, z2, zinv);
    fe_mul(x, R.x, z2);
    fe_mul(y, R.y, z3);
    fe_normalize(x);
    fe_normalize(y);
    bool same = true;
#pragma unroll
    for (int i = 0; i < 8; i++) same &= x.v[i] == q.v[i];
    return same && (y.v[0] & 1u) == parity;
}

// One whole row with an inversion of its own (host path, tests).
template <class GC>
BCC_HD int xonly_tweak_check_lane(const uint8_t* q32, u32 parity, const uint8_t* p32,
                                  const uint8_t* t32, const GC& gc) {
    fe p, q, tf, zinv;
    sc t;
    fe_from_be_bytes(p, p32);
    fe_from_be_bytes(q, q32);
    fe_from_be_bytes(tf, t32);
#pragma unroll
    for (int i = 0; i < 8; i++) t.v[i] = tf.v[i];
    gej R;
    const u32 st = tweak_add_lane(p, q, parity, t, gc, R);
    if (st != TC_NORMAL) return (int)st;
    fe_inv(zinv, R.z);
    return tweak_fin_lane(R, zinv, q, parity);
}

// ------------------------------------------------------------------------------------------
// host row builder: a batch of bcc_taproot_commit items -> the arrays the lanes read
// ------------------------------------------------------------------------------------------

// One lane's view of the round's blobs.  depth == COMMIT_SKIP: the control size is invalid and
// nothing is hashed (TAPROOT_WRONG_CONTROL_SIZE).
constexpr u32 COMMIT_SKIP = 0xFFFFFFFFu;
struct CommitLane {
    u32 leaf_blk;   // first 64-byte block of the padded leaf message in the leaf blob
    u32 leaf_nblk;
    u32 node_off;   // first 32-byte node in the node blob
    u32 depth;
};

constexpr unsigned COMMIT_CONTROL_BASE = 33, COMMIT_NODE = 32, COMMIT_MAX_NODES = 128;

inline bool commit_control_size_ok(unsigned len) {  // interpreter.cpp:1909-1911
    return len >= COMMIT_CONTROL_BASE && len <= COMMIT_CONTROL_BASE + COMMIT_NODE * COMMIT_MAX_NODES &&
           (len - COMMIT_CONTROL_BASE) % COMMIT_NODE == 0;
}
inline unsigned compact_size_len(unsigned n) { return n < 253 ? 1u : n <= 0xFFFFu ? 3u : 5u; }
// 64-byte blocks of the padded leaf message: version, compact size, script, 0x80, 8 length bytes
inline size_t commit_leaf_blocks(unsigned script_len) {
    return ((size_t)1 + compact_size_len(script_len) + script_len + 9 + 63) / 64;
}

// dst[0 .. 64 * commit_leaf_blocks(len)) = leaf_version || compact_size(len) || script || SHA-256
// padding for a message that follows the 64-byte tag prefix.
inline void commit_fill_leaf(uint8_t* dst, uint8_t leaf_version, const uint8_t* script, unsigned len) {
    const size_t total = 64 * commit_leaf_blocks(len);
    size_t o = 0;
    dst[o++] = leaf_version;
    if (len < 253) {
        dst[o++] = (uint8_t)len;
    } else if (len <= 0xFFFFu) {
        dst[o++] = 253;
        dst[o++] = (uint8_t)len;
        dst[o++] = (uint8_t)(len >> 8);
    } else {
        dst[o++] = 254;
        for (int i = 0; i < 4; i++) dst[o++] = (uint8_t)(len >> (8 * i));
    }
    if (len) memcpy(dst + o, script, len);
    o += len;
    const uint64_t bits = (uint64_t)(64 + o) * 8;
    dst[o++] = 0x80;
    memset(dst + o, 0, total - 8 - o);
    for (int i = 0; i < 8; i++) dst[total - 1 - i] = (uint8_t)(bits >> (8 * i));
}

// Pass 1 (serial, a few ns per item): every lane's place in the leaf and node blobs; returns the
// blobs' sizes in blocks / nodes.
inline void commit_plan(const bcc_taproot_commit* items, size_t n, CommitLane* lanes,
                        size_t* leaf_blocks, size_t* nodes) {
    size_t lb = 0, nd = 0;
    for (size_t i = 0; i < n; i++) {
        CommitLane& L = lanes[i];
        if (!commit_control_size_ok(items[i].control_len)) {
            L = CommitLane{0, 0, 0, COMMIT_SKIP};
            continue;
        }
        L.leaf_blk = (u32)lb;
        L.leaf_nblk = (u32)commit_leaf_blocks(items[i].script_len);
        L.node_off = (u32)nd;
        L.depth = (items[i].control_len - COMMIT_CONTROL_BASE) / COMMIT_NODE;
        lb += L.leaf_nblk;
        nd += L.depth;
    }
    *leaf_blocks = lb;
    *nodes = nd;
}

// Pass 2 for items [lo, hi) (any split over threads): the fixed-size rows p, q (32 bytes each) and
// the parity byte, the nodes and the padded leaf messages.  A skipped lane's rows are zero.
inline void commit_fill(const bcc_taproot_commit* items, const CommitLane* lanes, size_t lo, size_t hi,
                        uint8_t* p_row, uint8_t* q_row, uint8_t* par_row, uint8_t* node_blob,
                        uint8_t* leaf_blob) {
    for (size_t i = lo; i < hi; i++) {
        const bcc_taproot_commit& it = items[i];
        const CommitLane& L = lanes[i];
        if (L.depth == COMMIT_SKIP) {
            memset(p_row + 32 * i, 0, 32);
            memset(q_row + 32 * i, 0, 32);
            par_row[i] = 0;
            continue;
        }
        memcpy(p_row + 32 * i, it.control + 1, 32);
        memcpy(q_row + 32 * i, it.program32, 32);
        par_row[i] = it.control[0] & 1u;
        if (L.depth)
            memcpy(node_blob + (size_t)COMMIT_NODE * L.node_off, it.control + COMMIT_CONTROL_BASE,
                   (size_t)COMMIT_NODE * L.depth);
        commit_fill_leaf(leaf_blob + 64 * (size_t)L.leaf_blk, it.control[0] & 0xfeu, it.script,
                         it.script_len);
    }
}

// What the entry point reports for lane i given its curve verdict.
inline void commit_result(const CommitLane& L, int verdict, int* ret, int* serror) {
    if (L.depth == COMMIT_SKIP) {
        *ret = 0;
        *serror = BCC_SCRIPT_ERR_TAPROOT_WRONG_CONTROL_SIZE;
    } else {
        *ret = verdict ? 1 : 0;
        *serror = verdict ? 0 : BCC_SCRIPT_ERR_WITNESS_PROGRAM_MISMATCH;
    }
}

// One built lane on the host (small rounds, tests): the kernels' lane code with an inversion of
// its own.  leaf32 (optional) receives the TapLeaf hash, zeros for a skipped lane.
template <class GC>
inline void commit_host_lane(const CommitMids& m, const CommitLane* lanes, size_t i,
                             const uint8_t* p_row, const uint8_t* q_row, const uint8_t* par_row,
                             const uint8_t* node_blob, const uint8_t* leaf_blob, const GC& gc,
                             int* ret, int* serror, uint8_t* leaf32) {
    const CommitLane& L = lanes[i];
    int verdict = 0;
    if (L.depth == COMMIT_SKIP) {
        if (leaf32) memset(leaf32, 0, 32);
    } else {
        u32 leaf[8], t[8], raw[8];
        commit_hash_lane(m, reinterpret_cast<const u32*>(leaf_blob + 64 * (size_t)L.leaf_blk),
                         L.leaf_nblk,
                         reinterpret_cast<const u32*>(node_blob + (size_t)COMMIT_NODE * L.node_off),
                         L.depth, reinterpret_cast<const u32*>(p_row + 32 * i), leaf, t);
        store_be_words(raw, leaf);
        if (leaf32) memcpy(leaf32, raw, 32);
        store_be_words(raw, t);
        verdict = xonly_tweak_check_lane(q_row + 32 * i, par_row[i], p_row + 32 * i,
                                         reinterpret_cast<const uint8_t*>(raw), gc);
    }
    commit_result(L, verdict, ret, serror);
}

}  // namespace bcc
