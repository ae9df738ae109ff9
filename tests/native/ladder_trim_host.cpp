// tests/native/ladder_trim_host.cpp — TEST ONLY, a stand-alone program (its own main).  Drives the
// ladders' trimmed forms on the CPU -- the affine + affine first addition (gej_add_affine), the
// signed table read (get_pair with the digit's sign, -y stored in the Q table), the comb in
// extended Jacobian coordinates (twist_accumulate_g_xz) -- against the general forms they replace,
// restated here: every addition a gej_add_zinv into a Z = 1 start, the sign applied by fe_neg.  The
// two must give the same Jacobian coordinates mod p, not just the same point, so the comparison is
// on the normalised x, y, z and the infinity flag (the extended comb: the same point, ZZ^3 == ZZZ^2).
//
//   ladder_trim_host prims          direct primitive cases (exit status 0 = all passed)
//   ladder_trim_host ecdsa FILE     rows tag | x | y | r | s | m | verdict (162 bytes each)
//   ladder_trim_host schnorr FILE   rows sig64 | msg32 | pub32 | verdict   (129 bytes each)
#include "../../rust-bitcoinconsensus_amd/csrc/ecdsa_lane.h"
#include "../../rust-bitcoinconsensus_amd/csrc/ecdsa_twist.h"

#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace bcc;

static int g_fail = 0;
#define CHECK(c, ...)                                          \
    do {                                                       \
        if (!(c)) {                                            \
            if (g_fail++ < 20) {                               \
                printf("FAIL %s:%d %s ", __FILE__, __LINE__, #c); \
                printf(__VA_ARGS__);                           \
                printf("\n");                                  \
            }                                                  \
        }                                                      \
    } while (0)

static std::vector<fe>& gcomb() {
    static std::vector<fe> t;
    if (t.empty()) {
        t.resize((size_t)CWIN * CTAB * 2);
        build_g_comb(t.data());
    }
    return t;
}

static bool fe_same(fe a, fe b) {
    fe_normalize(a);
    fe_normalize(b);
    return memcmp(a.v, b.v, 32) == 0;
}
static bool gej_same(const gej& a, const gej& b) {
    return fe_same(a.x, b.x) && fe_same(a.y, b.y) && fe_same(a.z, b.z);
}

// e is the Jacobian point j: ZZ^3 == ZZZ^2 and the same affine point (a doubling inside the comb
// goes through another Z, so the coordinates themselves may differ by a scale)
static bool gexz_is(const gexz& e, const gej& j) {
    fe a, b, z2, z3;
    fe_sqr(a, e.zz);
    fe_mul(a, a, e.zz);
    fe_sqr(b, e.zzz);
    if (!fe_same(a, b) || fe_is_zero(e.zz)) return false;
    fe_sqr(z2, j.z);
    fe_mul(z3, z2, j.z);
    fe_mul(a, e.x, z2);
    fe_mul(b, j.x, e.zz);
    if (!fe_same(a, b)) return false;
    fe_mul(a, e.y, z3);
    fe_mul(b, j.y, e.zzz);
    return fe_same(a, b);
}
// ... and with the very coordinates: X, Y, ZZ = Z^2, ZZZ = Z^3
static bool gexz_exact(const gexz& e, const gej& j) {
    fe z2, z3;
    fe_sqr(z2, j.z);
    fe_mul(z3, z2, j.z);
    return fe_same(e.x, j.x) && fe_same(e.y, j.y) && fe_same(e.zz, z2) && fe_same(e.zzz, z3);
}

// ---- the forms the ladders had before: general additions from a Z = 1 start, fe_neg for the sign
static void old_pair(const QTableArray& qt, int i, int which, fe& x, fe& y) {
    qt.get(i, which, x);
    qt.get(i, 2, y);
}
template <class ST>
static bool old_accumulate_q(const ST& st, const QTableArray& qt, gej& acc) {
    const bool neg0 = (st.flags & LS_NEG0) != 0, neg1 = (st.flags & LS_NEG1) != 0;
    const fe one = fe_one();
    bool inf = false;
    {
        bool ng;
        u32 idx = digit_index(st.kword(0, 0), st.kword(0, 1), st.kword(0, 2), st.kword(0, 3), TOPQ,
                              WQ, TOPQ, ng);
        qt.get((int)idx, 0, acc.x);
        qt.get((int)idx, 2, acc.y);
        if (neg0) fe_neg(acc.y, acc.y);
        acc.z = one;
    }
    for (int pos = TOPQ; pos >= -1; pos--) {
        if (pos >= 0 && pos != TOPQ && !inf) {
            gej t;
            gej_double(t, acc);
            acc = t;
        }
        if (pos >= 0 && (pos % WQ) != 0) continue;
        for (int slot = 0; slot < 2; slot++) {
            const bool kneg = slot == 0 ? neg0 : neg1;
            u32 idx;
            bool sneg;
            if (pos >= 0) {
                if (slot == 0 && pos == TOPQ) continue;
                bool dneg;
                idx = digit_index(st.kword(slot, 0), st.kword(slot, 1), st.kword(slot, 2),
                                  st.kword(slot, 3), pos, WQ, TOPQ, dneg);
                sneg = dneg ^ kneg;
            } else {
                if (!(st.flags & (LS_CORR0 << slot))) continue;
                idx = 0;
                sneg = !kneg;
            }
            fe px, py;
            old_pair(qt, (int)idx, slot, px, py);
            if (sneg) fe_neg(py, py);
            acc_add(acc, inf, px, py, one, false);
        }
    }
    return inf;
}
template <class ST>
static bool old_accumulate_q_half(const ST& st, const QTableArray& qt, gej& acc, int slot) {
    const bool kneg = (st.flags & (slot == 0 ? LS_NEG0 : LS_NEG1)) != 0;
    const fe one = fe_one();
    bool inf = false;
    {
        bool ng;
        const u32 idx = digit_index(st.kword(slot, 0), st.kword(slot, 1), st.kword(slot, 2),
                                    st.kword(slot, 3), TOPQ, WQ, TOPQ, ng);
        old_pair(qt, (int)idx, slot, acc.x, acc.y);
        if (kneg) fe_neg(acc.y, acc.y);
        acc.z = one;
    }
    for (int pos = TOPQ; pos >= -1; pos--) {
        if (pos >= 0 && pos != TOPQ && !inf) {
            gej t;
            gej_double(t, acc);
            acc = t;
        }
        if (pos >= 0 && ((pos % WQ) != 0 || pos == TOPQ)) continue;
        u32 idx;
        bool sneg;
        if (pos >= 0) {
            bool dneg;
            idx = digit_index(st.kword(slot, 0), st.kword(slot, 1), st.kword(slot, 2),
                              st.kword(slot, 3), pos, WQ, TOPQ, dneg);
            sneg = dneg ^ kneg;
        } else {
            if (!(st.flags & (LS_CORR0 << slot))) continue;
            idx = 0;
            sneg = !kneg;
        }
        fe px, py;
        old_pair(qt, (int)idx, slot, px, py);
        if (sneg) fe_neg(py, py);
        acc_add(acc, inf, px, py, one, false);
    }
    return inf;
}
template <class ST>
static bool old_accumulate_g(const ST& st, const GCombArray& gc, gej& acc) {
    const fe one = fe_one();
    bool inf = false;
    {
        bool ng;
        u32 idx = comb_digit(st, WC * CTOP, ng);
        gc.get(CTOP, (int)idx, acc.x, acc.y);
        acc.z = one;
    }
    for (int win = CTOP - 1; win >= 0; win--) {
        bool neg;
        u32 idx = comb_digit(st, WC * win, neg);
        fe px, py;
        gc.get(win, (int)idx, px, py);
        if (neg) fe_neg(py, py);
        acc_add(acc, inf, px, py, one, false);
    }
    if (st.flags & LS_NEGU1) fe_neg(acc.y, acc.y);
    if (st.flags & LS_U1ZERO) inf = true;
    return inf;
}

// new against old on one prepared state: the whole Q ladder, both half ladders, the comb
static void compare_ladders(const TwistState& st, const QTableArray& qt, const char* what, size_t row) {
    GCombArray gc{gcomb().data()};
    gej a, b;
    bool ia = twist_accumulate_q(st, qt, a), ib = old_accumulate_q(st, qt, b);
    CHECK(ia == ib && gej_same(a, b), "%s row %zu: Q ladder", what, row);
    for (int slot = 0; slot < 2; slot++) {
        ia = twist_accumulate_q_half(st, qt, a, slot);
        ib = old_accumulate_q_half(st, qt, b, slot);
        CHECK(ia == ib && gej_same(a, b), "%s row %zu: Q half %d", what, row, slot);
    }
    ia = twist_accumulate_g(st, gc, a);
    ib = old_accumulate_g(st, gc, b);
    CHECK(ia == ib && gej_same(a, b), "%s row %zu: comb", what, row);
    gexz e;
    ia = twist_accumulate_g_xz(st, gc, e);
    CHECK(ia == ib && gexz_is(e, b), "%s row %zu: comb, extended Jacobian", what, row);
}

static void load32(fe& r, const unsigned char* p) { fe_from_be_bytes(r, p); }
static void load32(sc& r, const unsigned char* p) {
    fe t;
    fe_from_be_bytes(t, p);
    memcpy(r.v, t.v, 32);
}

static std::vector<unsigned char> slurp(const char* path) {
    std::vector<unsigned char> d;
    FILE* f = fopen(path, "rb");
    if (!f) return d;
    unsigned char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + n);
    fclose(f);
    return d;
}

static int run_ecdsa(const char* path) {
    const std::vector<unsigned char> d = slurp(path);
    const size_t R = 162, n = d.size() / R;
    if (n == 0 || d.size() % R) return 2;
    GCombArray gc{gcomb().data()};
    size_t ladders = 0;
    for (size_t i = 0; i < n; i++) {
        const unsigned char* p = d.data() + i * R;
        fe px, py;
        sc r, s, m;
        load32(px, p + 1);
        load32(py, p + 33);
        load32(r, p + 65);
        load32(s, p + 97);
        load32(m, p + 129);
        QTableArray qt;
        const int got = ecdsa_verify_twist_lane(p[0], px, py, r, s, m, qt, gc);
        CHECK(got == p[161], "ecdsa row %zu: verdict %d, expected %d", i, got, p[161]);
        QTableArray qh;
        const int goth = ecdsa_verify_twist_host(p[0], px, py, r, s, m, qh, gc);
        CHECK(goth == p[161], "ecdsa row %zu: host form verdict %d, expected %d", i, goth, p[161]);
        TwistState st;
        if (!twist_prep_lane(p[0], px, py, r, s, m, nullptr, qt, st)) continue;
        compare_ladders(st, qt, "ecdsa", i);
        ladders++;
    }
    printf("ecdsa: %zu rows, %zu ladders compared, %d failures\n", n, ladders, g_fail);
    return g_fail ? 1 : 0;
}

static int run_schnorr(const char* path) {
    const std::vector<unsigned char> d = slurp(path);
    const size_t R = 129, n = d.size() / R;
    if (n == 0 || d.size() % R) return 2;
    GCombArray gc{gcomb().data()};
    size_t ladders = 0;
    for (size_t i = 0; i < n; i++) {
        const unsigned char* p = d.data() + i * R;
        fe rx, px;
        sc s, m;
        load32(rx, p);
        load32(s, p + 32);
        load32(m, p + 64);
        load32(px, p + 96);
        QTableArray qt;
        const int got = schnorr_verify_twist_lane(px, rx, s, m, qt, gc);
        CHECK(got == p[128], "schnorr row %zu: verdict %d, expected %d", i, got, p[128]);
        TwistState st;
        if (!schnorr_twist_prep(px, rx, s, m, qt, st)) continue;
        compare_ladders(st, qt, "schnorr", i);
        ladders++;
    }
    printf("schnorr: %zu rows, %zu ladders compared, %d failures\n", n, ladders, g_fail);
    return g_fail ? 1 : 0;
}

// ---- direct primitive cases
static void rand_fe(std::mt19937_64& g, fe& a) {
    for (int i = 0; i < 8; i++) a.v[i] = (u32)g();
}

// a table of a real key: Q_w of the x-only key px (any x works: the formulas never use b)
static void table_of(std::mt19937_64& g, QTableArray& qt, fe& sigma) {
    fe px, v, qx, qy;
    rand_fe(g, px);
    curve_rhs(v, px);
    fe_mul(qx, px, v);
    fe_sqr(qy, v);
    build_q_table_coz(qx, qy, qt, sigma);
}

static int run_prims() {
    std::mt19937_64 g(0x1add37);
    const fe one = fe_one();
    // gej_add_affine against gej_add_zinv from Z = 1: distinct, equal and opposite points
    for (int it = 0; it < 200; it++) {
        QTableArray qt;
        fe sigma;
        table_of(g, qt, sigma);
        const int i = (int)(g() % QTAB), j = (int)(g() % QTAB);
        fe ax, ay, bx, by;
        qt.get_pair(i, 0, (g() & 1) != 0, ax, ay);
        qt.get_pair(j, (int)(g() & 1), (g() & 1) != 0, bx, by);
        const int mode = it % 4;  // 0, 1: as drawn (i == j with which == 0 gives a == +-b too)
        if (mode == 2) {          // equal: the doubling
            bx = ax;
            by = ay;
        } else if (mode == 3) {   // opposite: infinity, the result keeps a
            bx = ax;
            fe_neg(by, ay);
        }
        gej a, rn, ro;
        a.x = ax;
        a.y = ay;
        a.z = one;
        bool in = false, io = false;
        gej_add_affine(rn, in, ax, ay, bx, by);
        gej_add_zinv(ro, io, a, bx, by, one, false);
        CHECK(in == io && gej_same(rn, ro), "affine + affine, mode %d", mode);
        if (mode == 2) CHECK(!in, "equal points double");
        if (mode == 3) CHECK(in && gej_same(rn, a), "opposite points: infinity, r = a");
        // an infinity accumulator takes the next point as it is
        if (in) {
            fe cx, cy;
            qt.get_pair(j, 1, true, cx, cy);
            acc_add(rn, in, cx, cy, one, false);
            acc_add(ro, io, cx, cy, one, false);
            CHECK(!in && !io && gej_same(rn, ro) && fe_same(rn.x, cx) && fe_same(rn.y, cy) &&
                      fe_same(rn.z, one), "infinity accumulator");
        }
    }
    // every digit sign with every table index, both slots: (x or beta x, +-y)
    for (int it = 0; it < 8; it++) {
        QTableArray qt;
        fe sigma;
        table_of(g, qt, sigma);
        for (int i = 0; i < QTAB; i++)
            for (int which = 0; which < 2; which++)
                for (int neg = 0; neg < 2; neg++) {
                    fe x, y, ex, ey;
                    qt.get_pair(i, which, neg != 0, x, y);
                    old_pair(qt, i, which, ex, ey);
                    if (neg) fe_neg(ey, ey);
                    CHECK(fe_same(x, ex) && fe_same(y, ey), "get_pair(%d, %d, %d)", i, which, neg);
                    fe s;
                    qt.get(i, 2, ey);
                    qt.get(i, 3, y);
                    fe_add(s, y, ey);
                    CHECK(fe_is_zero(s), "stored -y of entry %d", i);
                }
    }
    // every flag combination (both halves' signs, both corrections) with every top and low digit
    // index: the ladders against their old forms on synthetic states
    for (int it = 0; it < 256; it++) {
        QTableArray qt;
        TwistState st;
        table_of(g, qt, st.sigma);
        st.flags = LS_VALID | (u32)((it & 15) << 1);  // LS_NEG0, LS_NEG1, LS_CORR0, LS_CORR0 << 1
        for (int q = 0; q < 4; q++)
            for (int w = 0; w < 4; w++) st.k[q][w] = (u32)g();
        st.k[0][0] |= 1u;
        st.k[1][0] |= 1u;
        st.k[2][0] |= 1u;
        // the top digit of each half takes every table index: bits 125..127
        st.k[0][3] = (st.k[0][3] & 0x1FFFFFFFu) | ((u32)((it >> 4) & 7) << 29);
        st.k[1][3] = (st.k[1][3] & 0x1FFFFFFFu) | ((u32)((it >> 5) & 7) << 29);
        if (it >= 128)  // and both halves start at the same entry
            st.k[1][3] = (st.k[1][3] & 0x1FFFFFFFu) | (st.k[0][3] & 0xE0000000u);
        compare_ladders(st, qt, "flags", (size_t)it);
    }
    // u1 == 0, u1 even, u1 odd through twist_prep_u1
    {
        QTableArray qt;
        TwistState st;
        table_of(g, qt, st.sigma);
        for (int w = 0; w < 4; w++) {
            st.k[0][w] = (u32)g();
            st.k[1][w] = (u32)g();
        }
        st.k[0][0] |= 1u;
        st.k[1][0] |= 1u;
        int seen = 0;
        for (int it = 0; it < 64; it++) {
            sc m, sinv;  // below 2^255 < n; the first m is 0
            for (int w = 0; w < 8; w++) {
                sinv.v[w] = (u32)g();
                m.v[w] = it > 0 ? (u32)g() : 0u;
            }
            sinv.v[7] &= 0x7FFFFFFFu;
            m.v[7] &= 0x7FFFFFFFu;
            st.flags = LS_VALID;
            twist_prep_u1(m, sinv, &st.flags, st.k[2], st.k[3]);
            seen |= (st.flags & LS_U1ZERO) ? 1 : (st.flags & LS_NEGU1) ? 2 : 4;
            compare_ladders(st, qt, "u1", (size_t)it);
        }
        CHECK(seen == 7, "u1 zero / even / odd all seen (%d)", seen);
    }
    // the extended-Jacobian mixed addition against gej_add_zinv: distinct points give the very
    // coordinates; the accumulator's own affine point doubles, its negative gives infinity
    {
        GCombArray gc{gcomb().data()};
        for (int it = 0; it < 60; it++) {
            fe ax, ay, bx, by, cx, cy;
            gc.get(3, (int)(g() % CTAB), ax, ay);
            gc.get(7, (int)(g() % CTAB), bx, by);
            gc.get(11, (int)(g() % CTAB), cx, cy);
            gej j, jr;
            gexz e, er;
            bool ij = false, ie = false;
            gej_add_affine(j, ij, ax, ay, bx, by);
            gexz_add_affine(e, ie, ax, ay, bx, by);
            CHECK(!ij && !ie && gexz_exact(e, j), "first addition, extended Jacobian");
            const int mode = it % 3;
            if (mode) {  // the accumulator's affine point, or its negative
                fe zi, zi2, zi3;
                fe_inv(zi, j.z);
                fe_sqr(zi2, zi);
                fe_mul(zi3, zi2, zi);
                fe_mul(cx, j.x, zi2);
                fe_mul(cy, j.y, zi3);
                if (mode == 2) fe_neg(cy, cy);
            }
            gej_add_zinv(jr, ij, j, cx, cy, one, false);
            gexz_add_ge(er, ie, e, cx, cy);
            CHECK(ij == ie && ie == (mode == 2), "extended Jacobian addition, mode %d: inf", mode);
            if (mode == 0) CHECK(gexz_exact(er, jr), "extended Jacobian addition");
            else CHECK(gexz_is(er, jr), "extended Jacobian addition, mode %d", mode);
            gej back;
            gexz_to_gej(back, er);
            CHECK(gexz_is(er, back), "extended Jacobian to Jacobian");
        }
    }
    // the first addition's exceptional branches on a comb point (on E itself)
    {
        GCombArray gc{gcomb().data()};
        fe ax, ay, ny;
        gc.get(CTOP, 5, ax, ay);
        fe_neg(ny, ay);
        gej r;
        bool inf = false;
        gej_add_affine(r, inf, ax, ay, ax, ny);
        CHECK(inf, "comb point + its negative");
        gej_add_affine(r, inf, ax, ay, ax, ay);
        gej a, d;
        a.x = ax;
        a.y = ay;
        a.z = one;
        gej_double(d, a);
        CHECK(!inf && gej_same(r, d), "comb point + itself");
    }
    printf("prims: %d failures\n", g_fail);
    return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "prims")) return run_prims();
    if (argc == 3 && !strcmp(argv[1], "ecdsa")) return run_ecdsa(argv[2]);
    if (argc == 3 && !strcmp(argv[1], "schnorr")) return run_schnorr(argv[2]);
    fprintf(stderr, "usage: %s prims | ecdsa FILE | schnorr FILE\n", argv[0]);
    return 2;
}
