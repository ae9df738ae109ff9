// The rule lanes of csrc/block_rules.h on the CPU, as a stand-alone program (test-only): reads the
// rows tests/test_block_rules_host.py wrote from the model and the fixture, runs the lane functions
// the kernels run and compares.  Built plainly and with -fsanitize=address,undefined.
//
//   script <hex or -> <sigops>
//   tx     <hex> <wit> <status> <n_in> <n_out> <sigops> <lock_time> <stripped> <coinbase> <all_final>
//   height <height> <hex of CScript() << height>
//   final  <lock_time> <all_final> <height> <cutoff> <0|1>
//   block  <hex> <height> <cutoff> <sigops> <stripped> <cb_first> <cb_later> <fail_tx> <fail_code>
//          <nonfinal_tx> <bip34_ok> <n_tx> then n_tx times <off> <len> <wit>
//
// Every transaction is walked through three byte sources: the plain one, the aligned-dword one the
// kernels use (over a copy at each of the four alignments inside a blob that ends as the round's raw
// blob does), and that one behind a checker which aborts on any read outside the transaction.  The
// duplicate lane runs with a serial compare-and-swap in every arrival order of up to six rows and
// in three orders above that.  Then 10,000 random byte strings as scripts and as transactions.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <numeric>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "block_rules.h"

using namespace bcc;

static std::vector<uint8_t> unhex(const std::string& s) {
    if (s == "-") return {};
    std::vector<uint8_t> out(s.size() / 2);
    for (size_t i = 0; i < out.size(); i++) out[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return out;
}

// Reads outside [lo, hi) end the program.
template <class Inner>
struct Checked {
    Inner in;
    uint32_t lo, hi;
    Checked(Inner i, uint32_t lo_, uint32_t hi_) : in(i), lo(lo_), hi(hi_) {}
    void must(bool ok, uint32_t pos, int k) {
        if (ok) return;
        fprintf(stderr, "read of %d at %u outside [%u, %u)\n", k, pos, lo, hi);
        abort();
    }
    uint32_t u8(uint32_t pos) {
        must(pos >= lo && pos < hi, pos, 1);
        return in.u8(pos);
    }
    uint32_t u32(uint32_t pos) {
        must(pos >= lo && hi - pos >= 4 && pos < hi, pos, 4);
        return in.u32(pos);
    }
};

// `bytes` at `shift` (0..3) + 4 * lead of a 4-aligned blob of exactly the dwords the round's raw
// blob has: the bytes, then four zero bytes, rounded up to whole dwords.
struct Blob {
    std::vector<uint32_t> words;
    uint32_t base;
    Blob(const std::vector<uint8_t>& bytes, uint32_t shift, uint32_t lead = 1) : base(4 * lead + shift) {
        words.assign((base + bytes.size() + 4 + 3) / 4, 0);
        memset(words.data(), 0xa5, base);
        if (!bytes.empty()) memcpy((uint8_t*)words.data() + base, bytes.data(), bytes.size());
    }
};

static bool same(const TxRuleRec& a, const TxRuleRec& b) {
    return a.n_in == b.n_in && a.n_out == b.n_out && a.stripped == b.stripped && a.sigops == b.sigops &&
           a.lock_time == b.lock_time && a.sig0_off == b.sig0_off && a.sig0_len == b.sig0_len &&
           a.is_coinbase == b.is_coinbase && a.all_final == b.all_final && a.before_dup == b.before_dup &&
           a.after_dup == b.after_dup;
}

// The lane through every source; the input rows of the aligned one (blob offsets) come back.
static TxRuleRec walk(const std::vector<uint8_t>& tx, uint32_t wit, size_t& bad, std::vector<InRow>* rows_out,
                      Blob* keep) {
    const uint32_t len = (uint32_t)tx.size(), cap = len / 41 + 1;
    std::vector<InRow> rows(cap), other(cap);
    PlainBytes p(tx.data());
    // (a vector's data() of an empty transaction may be null: the lane refuses len < 10 first)
    const TxRuleRec r = tx_rules_lane(p, 0, len, wit, rows.data(), cap, 7);
    for (uint32_t shift = 0; shift < 4; shift++) {
        Blob b(tx, shift);
        WordBytes w(b.words.data());
        const TxRuleRec rw = tx_rules_lane(w, b.base, len, wit, other.data(), cap, 7);
        Checked<WordBytes> c(WordBytes(b.words.data()), b.base, b.base + len);
        const TxRuleRec rc = tx_rules_lane(c, b.base, len, wit, other.data(), cap, 7);
        if (!same(r, rw) || !same(r, rc)) bad++;
        for (uint32_t k = 0; k < r.n_in && r.before_dup != TXR_MALFORMED; k++)
            if (other[k].off != rows[k].off + b.base || other[k].tx != 7) bad++;
        if (shift == 3 && keep) {
            *keep = b;
            if (rows_out) rows_out->assign(other.begin(), other.begin() + (r.before_dup == TXR_MALFORMED ? 0 : r.n_in));
        }
    }
    return r;
}

// The duplicate lane over `rows` of one blob, serially, rows arriving in `order`.
static bool dup_run(const Blob& b, const std::vector<InRow>& rows, const std::vector<uint32_t>& order,
                    uint32_t lo, uint32_t hi) {
    const uint32_t log2 = dup_table_log2(rows.size());
    std::vector<uint32_t> table((size_t)1 << log2, 0);
    auto cas = [](uint32_t* p, uint32_t expect, uint32_t v) {
        const uint32_t found = *p;
        if (found == expect) *p = v;
        return found;
    };
    bool dup = false;
    for (uint32_t me : order) {
        Checked<WordBytes> c(WordBytes(b.words.data()), lo, hi);
        dup |= dup_input_lane(c, rows.data(), (uint32_t)rows.size(), me, table.data(), log2, cas);
    }
    size_t used = 0;
    for (uint32_t w : table) used += w != 0;
    if (!dup && used != rows.size()) {  // every row of a duplicate-free table has its slot
        fprintf(stderr, "%zu rows took %zu slots\n", rows.size(), used);
        abort();
    }
    return dup;
}
static bool dup_all_orders(const Blob& b, const std::vector<InRow>& rows, uint32_t lo, uint32_t hi, size_t& bad,
                           std::mt19937& rng) {
    if (rows.size() < 2) return false;
    std::vector<uint32_t> order(rows.size());
    std::iota(order.begin(), order.end(), 0u);
    const bool first = dup_run(b, rows, order, lo, hi);
    if (rows.size() <= 6) {
        while (std::next_permutation(order.begin(), order.end()))
            if (dup_run(b, rows, order, lo, hi) != first) bad++;
    } else {
        std::reverse(order.begin(), order.end());
        if (dup_run(b, rows, order, lo, hi) != first) bad++;
        std::shuffle(order.begin(), order.end(), rng);
        if (dup_run(b, rows, order, lo, hi) != first) bad++;
    }
    return first;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line, kind;
    size_t rows = 0, bad = 0;
    std::mt19937 rng(20261022);
    auto fail = [&](const std::string& what) {
        if (bad++ < 10) std::cerr << "mismatch: " << what << "\n";
    };
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        if (!(ss >> kind)) continue;
        rows++;
        if (kind == "script") {
            std::string hex;
            uint32_t want;
            ss >> hex >> want;
            const std::vector<uint8_t> s = unhex(hex);
            for (uint32_t shift = 0; shift < 4; shift++) {
                Blob b(s, shift);
                Checked<WordBytes> c(WordBytes(b.words.data()), b.base, b.base + (uint32_t)s.size());
                if (script_sigops(c, b.base, (uint32_t)s.size()) != want) fail("script " + hex);
            }
            std::vector<uint8_t> copy(s);  // (its own allocation: a read past the end is the sanitizer's)
            PlainBytes p(copy.data());
            if (script_sigops(p, 0, (uint32_t)copy.size()) != want) fail("script, plain " + hex);
        } else if (kind == "tx") {
            std::string hex;
            uint32_t wit, status, n_in, n_out, sigops, lock, stripped, cb, fin;
            ss >> hex >> wit >> status >> n_in >> n_out >> sigops >> lock >> stripped >> cb >> fin;
            const std::vector<uint8_t> tx = unhex(hex);
            std::vector<InRow> irows;
            Blob b({}, 0);
            size_t before = bad;
            TxRuleRec r = walk(tx, wit, bad, &irows, &b);
            if (bad != before) fail("sources differ " + hex.substr(0, 40));
            r.dup = dup_all_orders(b, irows, b.base, b.base + (uint32_t)tx.size(), bad, rng) ? 1 : 0;
            if (tx_rule_code(r) != status || r.n_in != n_in || r.n_out != n_out || r.sigops != sigops ||
                r.lock_time != lock || r.stripped != stripped || r.is_coinbase != cb || r.all_final != fin)
                fail("tx " + hex.substr(0, 40) + " code " + std::to_string(tx_rule_code(r)));
        } else if (kind == "height") {
            int32_t h;
            std::string hex;
            ss >> h >> hex;
            uint8_t len, out[7];
            bip34_prefix(h, len, out);
            const std::vector<uint8_t> want = unhex(hex);
            if (len != want.size() || memcmp(out, want.data(), len) != 0) fail("height " + std::to_string(h));
        } else if (kind == "final") {
            TxRuleRec r{};
            uint32_t fin, want;
            int32_t height;
            int64_t cutoff;
            ss >> r.lock_time >> fin >> height >> cutoff >> want;
            r.all_final = (uint8_t)fin;
            if (tx_is_final(r, height, cutoff) != (want != 0)) fail("final " + line);
        } else if (kind == "block") {
            std::string hex;
            BlockRuleCtx c{};
            uint64_t sigops, stripped;
            uint32_t cb_first, cb_later, n;
            int64_t fail_tx, fail_code, nonfinal, bip34;
            ss >> hex >> c.height >> c.cutoff >> sigops >> stripped >> cb_first >> cb_later >> fail_tx >>
                fail_code >> nonfinal >> bip34 >> n;
            const std::vector<uint8_t> blk = unhex(hex);
            Blob b(blk, 1);
            std::vector<TxRuleRec> recs(n);
            std::vector<uint32_t> offs(n);
            for (uint32_t k = 0; k < n; k++) {
                uint32_t off, len, wit;
                ss >> off >> len >> wit;
                offs[k] = b.base + off;
                std::vector<InRow> irows(len / 41 + 1);
                Checked<WordBytes> s(WordBytes(b.words.data()), offs[k], offs[k] + len);
                recs[k] = tx_rules_lane(s, offs[k], len, wit, irows.data(), (uint32_t)irows.size(), k);
                irows.resize(recs[k].before_dup == TXR_MALFORMED ? 0 : recs[k].n_in);
                recs[k].dup = dup_all_orders(b, irows, offs[k], offs[k] + len, bad, rng) ? 1 : 0;
            }
            c.n_tx = n;
            bip34_prefix(c.height, c.bip34_len, c.bip34);
            // the block's transactions over 1, 3 and 64 lanes
            for (uint32_t lanes : {1u, 3u, 64u}) {
                BlockAcc a = block_rules_partial(recs.data(), c, 0, lanes);
                for (uint32_t l = 1; l < lanes; l++) block_acc_merge(a, block_rules_partial(recs.data(), c, l, lanes));
                Checked<WordBytes> s(WordBytes(b.words.data()), offs[0], b.base + (uint32_t)blk.size());
                const BlockRuleOut o = block_rules_finish(s, a, recs[0], offs[0], c);
                if (o.sigops != sigops || o.stripped != stripped || o.cb_first != cb_first || o.cb_later != cb_later ||
                    (int64_t)(int32_t)o.fail_tx != fail_tx || (int64_t)o.fail_code != fail_code ||
                    (int64_t)(int32_t)o.nonfinal_tx != nonfinal || (int64_t)o.bip34_ok != bip34)
                    fail("block of " + std::to_string(n) + " over " + std::to_string(lanes) + " lanes");
            }
        } else {
            fail("unknown row " + kind);
        }
    }
    // random bytes as scripts and as transactions: the sources agree and no read leaves the bytes
    size_t random_ok = 0;
    for (int k = 0; k < 10000; k++) {
        std::vector<uint8_t> s(rng() % 80);
        for (uint8_t& v : s) v = (rng() % 4 == 0) ? (uint8_t)(0x4b + rng() % 5) : (rng() % 3 == 0 ? (uint8_t)(0xac + rng() % 4) : (uint8_t)rng());
        std::vector<uint8_t> copy(s);
        PlainBytes p(copy.data());
        const uint32_t want = script_sigops(p, 0, (uint32_t)copy.size());
        Blob b(s, k & 3);
        Checked<WordBytes> c(WordBytes(b.words.data()), b.base, b.base + (uint32_t)s.size());
        if (script_sigops(c, b.base, (uint32_t)s.size()) != want) fail("random script");
        // a transaction: random bytes behind a plausible head, any witness offset the record check allows
        std::vector<uint8_t> t(10 + rng() % 200);
        for (uint8_t& v : t) v = (rng() % 3 == 0) ? (uint8_t)(rng() % 4) : (uint8_t)rng();
        if (k % 2) t[4] = 1 + rng() % 3;
        uint32_t wit = 0;
        if (k % 3 == 0 && t.size() >= 12) wit = 8 + rng() % (uint32_t)(t.size() - 4 - 8 + 1);
        const size_t before = bad;
        const TxRuleRec r = walk(t, wit, bad, nullptr, nullptr);
        if (bad != before) fail("random transaction");
        random_ok += r.before_dup != TXR_MALFORMED;
    }
    std::cout << rows << " rows, " << random_ok << " random transactions parsed, " << bad << " mismatches\n";
    return bad ? 1 : 0;
}
