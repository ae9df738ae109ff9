// Test-only, stand-alone: the arena layout function (arena.h) and the rule that makes a part's job
// records valid inside a concatenation of parts (pipeline.h PartBase / TapBase, rebase,
// part_starts, taproot_fill_part), on the host.
//
// usage: rebase_test [cases.txt]
// The layout checks need no input.  cases.txt (written by tests/test_rebase_rule.py from the
// committed goldens) holds one check per line, hex fields, "-" for an empty one:
//   E part dev|host sigversion hashtype nin amount tx code sighash
//   H part row                                  a key-hash record on that row of the part
//   T part dev|host sigversion nin codesep tx spent sig pk annex tapleaf sighash ret
// "dev" checks go through the product's job builders (build_sighash_checks with the device hash
// types on; taproot_add_check); "host" checks become host-preimage jobs (build_sighash_checks with
// the switch off, transplanted behind the part's rows by hand) and hand-built Taproot SigMsgs with
// their five aux messages and patches.  Each part is evaluated alone by the host evaluation, the
// parts are merged (append_round; taproot_fill_part) and evaluated again: the digests must agree
// byte for byte with each other and with the goldens' reference digests.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "arena.h"
#include "bcc_amd.h"
#include "host/engine.h"
#include "host/host_verify.h"
#include "host/taproot_host.h"
#include "host/taproot_jobs.h"
#include "host/tx.h"
#include "pipeline.h"

using namespace bcc;
using Bytes = std::vector<uint8_t>;

static int g_failed = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            g_failed++;                                                          \
        }                                                                        \
    } while (0)

// ---- the layout function ---------------------------------------------------------------------

static void check_layout(const std::vector<size_t>& sizes) {
    const int nb = (int)sizes.size();
    std::vector<size_t> off(nb + 1, 12345);
    const size_t total = arena_layout(sizes.data(), off.data(), nb);
    CHECK(off[0] == 0);
    CHECK(off[nb] == total);
    for (int i = 0; i < nb; i++) {
        CHECK(off[i] % 256 == 0);
        CHECK(off[i + 1] >= off[i]);
        CHECK(off[i + 1] - off[i] >= sizes[i]);       // the region holds its bytes
        CHECK(off[i + 1] - off[i] < sizes[i] + 256);  // and no more than the alignment asks
        if (sizes[i] == 0) CHECK(off[i + 1] == off[i]);
    }
    CHECK(total % 256 == 0);
}

static void test_layout() {
    check_layout({0, 0, 0});
    check_layout({1});
    check_layout({256});
    check_layout({257});
    check_layout({5, 0, 300});
    check_layout({0, 1, 256, 257, 0, 0, 511, 512, 513, 0});
    size_t off[4];
    const size_t s[3] = {5, 0, 300};
    CHECK(arena_layout(s, off, 3) == 256 + 512);
    CHECK(off[1] == 256 && off[2] == 256 && off[3] == 768);
    const size_t z[2] = {0, 0};
    CHECK(arena_layout(z, off, 2) == 0);
    CHECK(align256(0) == 0 && align256(1) == 256 && align256(256) == 256 && align256(257) == 512);
}

// ---- input -----------------------------------------------------------------------------------

static Bytes unhex(const std::string& s) {
    Bytes b;
    if (s == "-") return b;
    for (size_t i = 0; i + 1 < s.size(); i += 2) b.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return b;
}

// one buffer per distinct blob: checks of the same tx share its pointer, as a batch's items do
static const Bytes& blob(const std::string& hex) {
    static std::map<std::string, std::unique_ptr<Bytes>> pool;
    auto& p = pool[hex];
    if (!p) p = std::make_unique<Bytes>(unhex(hex));
    return *p;
}

struct ECheck {
    int sigversion, hashtype;
    unsigned nin;
    int64_t amount;
    const Bytes *tx, *code;
    Bytes expect;
};
struct TCheck {
    bool dev;
    int sigversion;
    unsigned nin;
    uint32_t codesep;
    const Bytes *tx, *spent, *sig, *pk, *annex, *leaf;
    Bytes expect;
    int ret;
};
constexpr int PARTS = 3;
struct Cases {
    std::vector<ECheck> edev[PARTS], ehost[PARTS];
    std::vector<uint32_t> hrow[PARTS];
    std::vector<TCheck> tap[PARTS];
};

static bool read_cases(const char* path, Cases& c) {
    std::ifstream f(path);
    if (!f) return false;
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string kind, mode, tx, code, expect, spent, sig, pk, annex, leaf;
        int part = 0;
        if (!(in >> kind >> part) || part < 0 || part >= PARTS) continue;
        if (kind == "E") {
            ECheck e{};
            in >> mode >> e.sigversion >> e.hashtype >> e.nin >> e.amount >> tx >> code >> expect;
            e.tx = &blob(tx);
            e.code = &blob(code);
            e.expect = unhex(expect);
            (mode == "dev" ? c.edev : c.ehost)[part].push_back(e);
        } else if (kind == "H") {
            uint32_t row = 0;
            in >> row;
            c.hrow[part].push_back(row);
        } else if (kind == "T") {
            TCheck t{};
            in >> mode >> t.sigversion >> t.nin >> t.codesep >> tx >> spent >> sig >> pk >> annex >> leaf >>
                expect >> t.ret;
            t.dev = mode == "dev";
            t.tx = &blob(tx);
            t.spent = &blob(spent);
            t.sig = &blob(sig);
            t.pk = &blob(pk);
            t.annex = annex == "-" ? nullptr : &blob(annex);
            t.leaf = leaf == "-" ? nullptr : &blob(leaf);
            t.expect = unhex(expect);
            c.tap[part].push_back(t);
        }
        if (!in) return false;
    }
    return true;
}

// ---- ECDSA-era records -------------------------------------------------------------------------

static bool build(const std::vector<ECheck>& cs, bool device_hashtypes, SighashJobs& J, TupleRows& R) {
    std::vector<host::SighashCheck> sc;
    for (const ECheck& e : cs)
        sc.push_back(host::SighashCheck{e.tx->data(), e.tx->size(), e.code->data(), e.code->size(), e.nin,
                                        e.hashtype, e.amount, e.sigversion});
    bcc_set_device_hashtypes(device_hashtypes ? 1 : 0);
    const size_t n = host::build_sighash_checks(sc.data(), sc.size(), J, R);
    bcc_set_device_hashtypes(0);
    return n == cs.size() && R.size() == cs.size();
}

// host_sighash over rows initialised to ONE (what a device round's rows hold before the kernels)
static Bytes digests(const SighashJobs& J, size_t rows) {
    Bytes msg(32 * rows, 0);
    for (size_t i = 0; i < rows; i++) msg[32 * i] = 1;
    host::host_sighash(J, msg.data());
    return msg;
}

static void mark_rows(TupleRows& R, int part) {  // a row's x names its part and place
    for (size_t r = 0; r < R.size(); r++) {
        R.x[32 * r] = (uint8_t)(part + 1);
        R.x[32 * r + 1] = (uint8_t)r;
        R.x[32 * r + 2] = (uint8_t)(r >> 8);
    }
}

static void test_sighash_parts(const Cases& c) {
    SighashJobs J[PARTS];
    TupleRows R[PARTS];
    Bytes expect;
    for (int p = 0; p < PARTS; p++) {
        CHECK(build(c.edev[p], true, J[p], R[p]));
        CHECK(J[p].pre_off.empty() && J[p].aux_off.empty() && J[p].patches.empty());
        for (const ECheck& e : c.edev[p]) expect.insert(expect.end(), e.expect.begin(), e.expect.end());
        if (!c.ehost[p].empty()) {
            // the host-preimage jobs of these checks, behind the part's rows by hand: the part has
            // no preimage or aux message yet, so only the rows move
            SighashJobs hj;
            TupleRows hr;
            CHECK(build(c.ehost[p], false, hj, hr));
            CHECK(hj.tjobs.empty() && hj.wjobs.empty() && hj.ljobs.empty());
            const uint32_t k = (uint32_t)R[p].size();
            J[p].pre = hj.pre; J[p].pre_off = hj.pre_off; J[p].pre_nblk = hj.pre_nblk;
            for (uint32_t r : hj.pre_row) J[p].pre_row.push_back(r + k);
            J[p].aux = hj.aux; J[p].aux_off = hj.aux_off; J[p].aux_nblk = hj.aux_nblk;
            J[p].patches = hj.patches;
            const uint8_t zero[32] = {0};
            uint8_t one[32] = {1};
            for (size_t r = 0; r < hr.size(); r++) R[p].add(0x02, zero, zero, zero, zero, one);
            for (const ECheck& e : c.ehost[p]) expect.insert(expect.end(), e.expect.begin(), e.expect.end());
        }
        mark_rows(R[p], p);
        const uint8_t prog[20] = {(uint8_t)p};
        for (uint32_t r : c.hrow[p]) {
            CHECK(r < R[p].size());
            R[p].add_key_hash(r, prog);
        }
    }
    // what the parts must hold: every record kind across them, nothing in the middle part, and no
    // LinJob, host preimage or key-hash record in the last
    size_t mid = 0, nomid = 0, win = 0, single = 0;
    for (int p = 0; p < PARTS; p++) {
        for (const TplJob& t : J[p].tjobs) (tpl_has_mid(t) ? mid : nomid)++;
        for (const WinJob& w : J[p].wjobs) ((w.hashtype & 0x1f) == 3 ? single : win)++;
    }
    CHECK(mid && nomid && win && single);
    CHECK(!J[0].ljobs.empty() && !J[0].pre_off.empty() && !J[0].patches.empty() && !J[0].aux_off.empty());
    CHECK(J[0].pre_off.size() >= 2 && J[0].aux_off.size() >= 2);  // a later preimage / aux to rebase
    CHECK(!R[0].hrow.empty());
    CHECK(J[0].wtx.size() >= 2 && J[2].wtx.size() >= 2);  // a tx index above zero to rebase
    CHECK(R[1].size() == 0 && J[1].tjobs.empty() && J[1].wjobs.empty() && J[1].ljobs.empty() &&
          J[1].pre_off.empty() && J[1].wtx.empty() && J[1].code.empty() && R[1].hrow.empty());
    CHECK(!J[2].tjobs.empty() && !J[2].wjobs.empty() && J[2].n_win_single != 0);
    CHECK(J[2].ljobs.empty() && J[2].pre_off.empty() && J[2].aux_off.empty() && R[2].hrow.empty());

    Bytes apart;
    for (int p = 0; p < PARTS; p++) {
        const Bytes d = digests(J[p], R[p].size());
        apart.insert(apart.end(), d.begin(), d.end());
    }
    SighashJobs MJ;
    TupleRows MR;
    for (int p = 0; p < PARTS; p++) host::append_round(MJ, MR, J[p], R[p]);
    const Bytes merged = digests(MJ, MR.size());
    CHECK(apart.size() == expect.size() && !expect.empty());
    CHECK(apart == merged);
    CHECK(apart == expect);

    // the parts' starts agree with what the merge produced, and carry the key-hash rows to the
    // rows they named (the merge above does not take hrow along: staging does, by this rule)
    const SighashJobs* jp[PARTS] = {&J[0], &J[1], &J[2]};
    const TupleRows* rp[PARTS] = {&R[0], &R[1], &R[2]};
    const std::vector<PartExtent> at = part_starts(jp, rp, PARTS);
    const PartExtent& T = at[PARTS];
    CHECK(T.row == MR.size() && T.aux_bytes == MJ.aux.size() && T.pre_bytes == MJ.pre.size() &&
          T.aux_idx == MJ.aux_off.size() && T.pre_idx == MJ.pre_off.size() &&
          T.patch == MJ.patches.size() && T.tpl == MJ.tpl.size() && T.code == MJ.code.size() &&
          T.tjob == MJ.tjobs.size() && T.raw == MJ.txraw.size() && T.wtx == MJ.wtx.size() &&
          T.wjob == MJ.wjobs.size() && T.ljob == MJ.ljobs.size() && T.win == MJ.win_entries);
    CHECK(at[1].row == at[2].row && at[1].code == at[2].code && at[1].hrow == at[2].hrow);  // empty part
    std::vector<uint32_t> hrow(T.hrow, 0xFFFFFFFFu);
    for (int p = 0; p < PARTS; p++)
        rebase_copy(hrow.data() + at[p].hrow, R[p].hrow.data(), R[p].hrow.size(), part_base(at[p]).row);
    for (int p = 0; p < PARTS; p++)
        for (size_t k = 0; k < R[p].hrow.size(); k++) {
            const uint32_t m = hrow[at[p].hrow + k], r = R[p].hrow[k];
            CHECK(m < MR.size());
            CHECK(MR.x[32 * m] == p + 1 && MR.x[32 * m + 1] == (uint8_t)r && MR.x[32 * m + 2] == (uint8_t)(r >> 8));
        }
    // every record's row lands on the row it named
    for (int p = 0; p < PARTS; p++) {
        for (size_t k = 0; k < J[p].tjobs.size(); k++) {
            const uint32_t m = MJ.tjobs[at[p].tjob + k].row;
            CHECK(MR.x[32 * m] == p + 1 && MR.x[32 * m + 1] == (uint8_t)J[p].tjobs[k].row);
        }
        for (size_t k = 0; k < J[p].ljobs.size(); k++) {
            const uint32_t m = MJ.ljobs[at[p].ljob + k].row;
            CHECK(MR.x[32 * m] == p + 1 && MR.x[32 * m + 1] == (uint8_t)J[p].ljobs[k].row);
        }
    }
}

// ---- Taproot records ---------------------------------------------------------------------------

static void le32(Bytes& b, uint32_t v) {
    for (int i = 0; i < 4; i++) b.push_back((uint8_t)(v >> (8 * i)));
}

// A host-built check by hand: the BIP341 SigMsg of a SIGHASH_DEFAULT / SIGHASH_ALL signature with
// zeroed slots for sha_prevouts / sha_amounts / sha_scriptpubkeys / sha_sequences / sha_outputs,
// the five messages those are the SHA-256 of, and the patches that carry the digests over.
static bool add_host_built(TaprootJobs& J, const TCheck& t) {
    host::Tx tx;
    std::vector<host::TxOut> outs;
    if (!host::parse_tx(t.tx->data(), t.tx->size(), tx) ||
        !host::parse_txouts(t.spent->data(), t.spent->size(), outs) || outs.size() != tx.vin.size())
        return false;
    if (t.annex || (t.sig->size() != 64 && !(t.sig->size() == 65 && (*t.sig)[64] == 1))) return false;
    Bytes aux[5];
    for (size_t i = 0; i < tx.vin.size(); i++) {
        aux[0].insert(aux[0].end(), tx.vin[i].prevout, tx.vin[i].prevout + 36);
        for (int b = 0; b < 8; b++) aux[1].push_back((uint8_t)((uint64_t)outs[i].value >> (8 * b)));
        aux[2].insert(aux[2].end(), outs[i].ser.p + 8, outs[i].ser.end());
        le32(aux[3], tx.vin[i].sequence);
    }
    for (const host::TxOut& o : tx.vout) aux[4].insert(aux[4].end(), o.ser.p, o.ser.end());
    const bool tapscript = t.sigversion == BCC_SIGVERSION_TAPSCRIPT;
    Bytes m;
    m.push_back(0);  // epoch
    m.push_back(t.sig->size() == 65 ? 1 : 0);
    le32(m, (uint32_t)tx.version);
    le32(m, tx.locktime);
    const size_t slot0 = m.size();
    m.resize(m.size() + 160, 0);
    m.push_back(tapscript ? 2 : 0);  // spend_type: ext_flag << 1, no annex
    le32(m, t.nin);
    if (tapscript) {
        if (!t.leaf) return false;
        m.insert(m.end(), t.leaf->begin(), t.leaf->end());
        m.push_back(0);  // key_version
        le32(m, t.codesep);
    }
    const uint32_t row = (uint32_t)J.rows();
    const uint32_t k = J.add_msg(m.data(), m.size(), row);
    for (int a = 0; a < 5; a++) {
        const uint32_t ai = J.add_aux(aux[a].data(), aux[a].size());
        J.patches.push_back(PatchRec{(uint32_t)(J.msg_off[k] * 64 + slot0 + 32 * a), ai});
    }
    J.sig64.insert(J.sig64.end(), t.sig->begin(), t.sig->begin() + 64);
    J.pk32.insert(J.pk32.end(), t.pk->begin(), t.pk->end());
    return true;
}

static void test_taproot_parts(const Cases& c) {
    TaprootJobs J[PARTS];
    Bytes expect, expect_v;
    Bytes scratch;
    for (int p = 0; p < PARTS; p++) {
        host::TxState s;
        for (const TCheck& t : c.tap[p]) {
            if (t.dev) {
                CHECK(host::load_tx(s, t.tx->data(), (unsigned)t.tx->size(), t.spent->data(),
                                    (unsigned)t.spent->size()));
                CHECK(host::taproot_add_check(s, J[p], t.nin, t.sig->data(), (unsigned)t.sig->size(),
                                              t.pk->data(), t.sigversion == BCC_SIGVERSION_TAPSCRIPT,
                                              t.annex ? t.annex->data() : nullptr,
                                              t.annex ? (unsigned)t.annex->size() : 0,
                                              t.leaf ? t.leaf->data() : nullptr, t.codesep, scratch) == 0);
            } else {
                CHECK(add_host_built(J[p], t));
            }
            expect.insert(expect.end(), t.expect.begin(), t.expect.end());
            expect_v.push_back(t.ret == 1 ? 1 : 0);
        }
    }
    CHECK(!J[0].msg_off.empty() && !J[0].patches.empty() && !J[0].dev.jobs.empty());  // both kinds
    CHECK(J[0].dev.ttx.size() >= 2 && !J[0].dev.ext.empty());
    CHECK(J[1].rows() == 0 && J[1].msg_off.empty() && J[1].dev.jobs.empty() && J[1].dev.txraw.empty());
    CHECK(J[2].msg_off.empty() && J[2].aux_off.empty() && !J[2].dev.jobs.empty() && !J[2].dev.ext.empty());

    const TaprootJobs* parts[PARTS] = {&J[0], &J[1], &J[2]};
    const std::vector<TapExtent> at = part_starts(parts, PARTS);
    const TapExtent& T = at[PARTS];
    const size_t n = T.row;
    CHECK(n == expect_v.size() && n != 0);
    Bytes v1(n, 9), m1(32 * n, 0), v2(n, 9), m2(32 * n, 0);
    host::host_taproot_parts(parts, PARTS, v1.data(), m1.data(), 1);

    TaprootJobs M;  // the concatenation, written by the function the device round fills its image with
    M.sig64.resize(64 * n); M.pk32.resize(32 * n);
    M.aux.resize(T.aux_bytes); M.msg.resize(T.msg_bytes);
    M.aux_off.resize(T.aux_idx); M.aux_nblk.resize(T.aux_idx);
    M.msg_off.resize(T.msg_idx); M.msg_nblk.resize(T.msg_idx); M.msg_row.resize(T.msg_idx);
    M.patches.resize(T.patch);
    M.dev.txraw.resize(T.raw); M.dev.ext.resize(T.ext); M.dev.ttx.resize(T.ttx); M.dev.jobs.resize(T.tjob);
    M.dev.in_entries = (uint32_t)T.in;
    const TapImage im{M.sig64.data(), M.pk32.data(), M.aux.data(), M.msg.data(),
                      M.aux_off.data(), M.aux_nblk.data(), M.msg_off.data(), M.msg_nblk.data(),
                      M.msg_row.data(), M.patches.data(), M.dev.txraw.data(), M.dev.ext.data(),
                      M.dev.ttx.data(), M.dev.jobs.data()};
    for (int p = 0; p < PARTS; p++) taproot_fill_part(im, J[p], at[p]);
    const TaprootJobs* mp = &M;
    host::host_taproot_parts(&mp, 1, v2.data(), m2.data(), 1);
    CHECK(v1 == v2);
    CHECK(m1 == m2);
    CHECK(m1 == expect);
    CHECK(v1 == expect_v);
}

int main(int argc, char** argv) {
    test_layout();
    if (argc > 1) {
        Cases c;
        if (!read_cases(argv[1], c)) {
            fprintf(stderr, "cannot read %s\n", argv[1]);
            return 2;
        }
        test_sighash_parts(c);
        test_taproot_parts(c);
    }
    if (g_failed) {
        fprintf(stderr, "%d check(s) failed\n", g_failed);
        return 1;
    }
    printf("rebase_test ok%s\n", argc > 1 ? "" : " (layout only)");
    return 0;
}
