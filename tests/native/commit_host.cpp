// tests/native/commit_host.cpp — TEST ONLY. Runs the product's script-path commitment lane code
// and host row builder (rust-bitcoinconsensus_amd/csrc/taproot_commit.h) on the CPU, so the exact
// arithmetic of the HIP kernels and the rows they read can be checked against the reference
// without a GPU. Never linked into the product.
#include "../../rust-bitcoinconsensus_amd/csrc/taproot_commit.h"

#include <vector>

using namespace bcc;

static std::vector<fe>& gcomb() {
    static std::vector<fe> t;
    if (t.empty()) {
        t.resize((size_t)CWIN * CTAB * 2);
        build_g_comb(t.data());
    }
    return t;
}

// bcc_taproot_commit_batch's contract through commit_plan / commit_fill / commit_host_lane.
// `split` > 1 fills the rows in that many separate ranges, as the engine's worker team does.
extern "C" int commit_host_batch(const bcc_taproot_commit* items, size_t n, int* ret, int* serror,
                                 unsigned char* tapleaf, unsigned split) {
    std::vector<CommitLane> lanes(n);
    size_t lb = 0, nd = 0;
    commit_plan(items, n, lanes.data(), &lb, &nd);
    std::vector<u32> pw(8 * n + 1), qw(8 * n + 1), nodes(8 * nd + 1), leaf(16 * lb + 1);
    std::vector<uint8_t> par(n + 1);
    uint8_t *p = (uint8_t*)pw.data(), *q = (uint8_t*)qw.data(), *nb = (uint8_t*)nodes.data(),
            *lf = (uint8_t*)leaf.data();
    if (split < 1) split = 1;
    for (unsigned s = split; s-- > 0;)  // back to front: the ranges are independent
        commit_fill(items, lanes.data(), n * s / split, n * (s + 1) / split, p, q, par.data(), nb, lf);
    GCombArray gc{gcomb().data()};
    const CommitMids m = commit_mids();
    for (size_t i = 0; i < n; i++)
        commit_host_lane(m, lanes.data(), i, p, q, par.data(), nb, lf, gc, ret + i, serror + i,
                         tapleaf ? tapleaf + 32 * i : nullptr);
    return 0;
}

// mi_xonly_tweak_check_tuples' contract, one inversion per row.
extern "C" void commit_tweak_check(const unsigned char* q32, const unsigned char* parity,
                                   const unsigned char* p32, const unsigned char* t32,
                                   unsigned char* verdict, size_t n) {
    GCombArray gc{gcomb().data()};
    for (size_t i = 0; i < n; i++)
        verdict[i] = (unsigned char)xonly_tweak_check_lane(q32 + 32 * i, parity[i], p32 + 32 * i,
                                                           t32 + 32 * i, gc);
}

// The same rows with the kernels' grouping: tweak_add_lane per row, then one inversion per group of
// `group` rows strided by T = ceil(n / group) (Montgomery's trick exactly as tweak_fin_kernel walks
// it), decided rows leaving the product alone.
extern "C" void commit_tweak_check_grouped(const unsigned char* q32, const unsigned char* parity,
                                           const unsigned char* p32, const unsigned char* t32,
                                           unsigned char* verdict, size_t n, size_t group) {
    GCombArray gc{gcomb().data()};
    std::vector<gej> R(n);
    std::vector<fe> pre(n), qs(n);
    std::vector<u32> stat(n);
    for (size_t i = 0; i < n; i++) {
        fe p, tf;
        sc t;
        fe_from_be_bytes(p, p32 + 32 * i);
        fe_from_be_bytes(qs[i], q32 + 32 * i);
        fe_from_be_bytes(tf, t32 + 32 * i);
        for (int j = 0; j < 8; j++) t.v[j] = tf.v[j];
        stat[i] = tweak_add_lane(p, qs[i], parity[i], t, gc, R[i]);
    }
    const size_t T = (n + group - 1) / group;
    for (size_t t = 0; t < T && t < n; t++) {
        fe acc = fe_one();
        size_t last = t;
        for (size_t i = t; i < n; i += T) {
            if (stat[i] == TC_NORMAL) {
                pre[i] = acc;
                fe_mul(acc, acc, R[i].z);
            }
            last = i;
        }
        fe inv;
        fe_inv(inv, acc);
        for (size_t i = last + T; i > t;) {
            i -= T;
            int ok = stat[i] == TC_TRUE;
            if (stat[i] == TC_NORMAL) {
                fe zinv;
                fe_mul(zinv, inv, pre[i]);
                fe_mul(inv, inv, R[i].z);
                ok = tweak_fin_lane(R[i], zinv, qs[i], parity[i]);
            }
            verdict[i] = (unsigned char)ok;
        }
    }
}
