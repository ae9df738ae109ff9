// The job builder of the BIP341 / BIP342 signature checks, shared by bcc_taproot_verify_batch
// (taproot.cpp) and bcc_taproot_spend_batch (taproot_spend.cpp): the parsed tx an adjacent run of
// items shares, its record in a part's device blobs, and one check's rules and TapJob.
#pragma once
#include <cstdint>
#include <vector>

#include "../pipeline.h"
#include "bcc_amd.h"
#include "hashes.h"
#include "tx.h"

namespace bcc {
namespace host {

// The parsed tx (and spent outputs) an adjacent run of items shares, and its TtxRec in the
// current part.
struct TxState {
    const uint8_t* tx = nullptr;
    unsigned tx_len = 0;
    const uint8_t* spent = nullptr;
    unsigned spent_len = 0;
    bool ok = false;      // parsed, and the tx data would be BIP341-ready
    bool parsed = false;  // the tx and its spent outputs deserialize and match in count
    Tx t;
    std::vector<TxOut> outs;
    int32_t ttx = -1;  // TtxRec index in the current part (-1: not added yet)
};

// The tx (without marker, flag and witnesses: the SigMsg kernels never read them) and the outputs
// it spends, once per part.
inline uint32_t tx_record(TxState& s, TaprootTxJobs& D) {
    if (s.ttx >= 0) return (uint32_t)s.ttx;
    TtxRec r{};
    r.tx_off = (uint32_t)D.txraw.size();
    const uint8_t* raw = s.tx;
    const size_t len = s.tx_len;
    if (s.t.has_witness() && !s.t.vout.empty() && len > 10) {  // BIP144: inputs start at byte 6
        const Span& last = s.t.vout.back().ser;
        const size_t mid = (size_t)(last.p + last.n - (raw + 6));
        D.put_raw(raw, 4);
        D.put_raw(raw + 6, mid);
        D.put_raw(raw + len - 4, 4);
        r.tx_len = (uint32_t)(8 + mid);
    } else {
        D.put_raw(raw, len);
        r.tx_len = (uint32_t)len;
    }
    D.align4();
    r.sp_off = (uint32_t)D.txraw.size();
    r.sp_len = s.spent_len;
    D.put_raw(s.spent, s.spent_len);
    D.align4();
    r.in_base = D.in_entries;
    r.n_in = (uint32_t)s.t.vin.size();
    D.in_entries += r.n_in;
    D.ttx.push_back(r);
    s.ttx = (int32_t)D.ttx.size() - 1;
    return (uint32_t)s.ttx;
}

inline bool load_tx(TxState& s, const uint8_t* tx, unsigned tx_len, const uint8_t* spent,
                    unsigned spent_len) {
    if (s.tx == tx && s.tx_len == tx_len && s.spent == spent && s.spent_len == spent_len && s.tx)
        return s.ok;
    s.tx = tx;
    s.tx_len = tx_len;
    s.spent = spent;
    s.spent_len = spent_len;
    s.ttx = -1;
    s.ok = s.parsed = tx && spent && parse_tx(tx, tx_len, s.t) && s.t.ser_size == tx_len &&
                      parse_txouts(spent, spent_len, s.outs) && s.outs.size() == s.t.vin.size();
    if (s.ok) {
        // m_bip341_taproot_ready (interpreter.cpp:1436-1452); SignatureHashSchnorr asserts it
        bool ready = false;
        for (size_t i = 0; i < s.t.vin.size() && !ready; i++)
            ready = !s.t.vin[i].witness.empty() && s.outs[i].script.size() == 34 &&
                    s.outs[i].script.p[0] == 0x51;
        s.ok = ready;
    }
    return s.ok;
}

// One check of GenericTransactionSignatureChecker::CheckSchnorrSignature (interpreter.cpp:1688-1700)
// on input n_in of the loaded tx: the size / hash_type rules and SignatureHashSchnorr's early
// returns (:1523, :1557) on the host, returning their BCC_SCRIPT_ERR_* code; else 0, and the check
// is row J.rows() of the part: its TapJob (the SigMsg is assembled on the device by
// taproot_msg_kernel from the tx bytes), signature and key.  leaf32 = the tapleaf hash of a
// tapscript check, or nullptr when a later stage writes it into the job's ext slot (32 zero bytes
// are reserved).  The slot's byte offset in J.dev.ext goes to *leaf_slot when given.
inline int taproot_add_check(TxState& s, TaprootJobs& J, unsigned n_in, const uint8_t* sig,
                             unsigned sig_len, const uint8_t* pk32, bool tapscript,
                             const uint8_t* annex, unsigned annex_len, const uint8_t* leaf32,
                             uint32_t codesep, std::vector<uint8_t>& scratch,
                             uint32_t* leaf_slot = nullptr) {
    if (sig_len != 64 && sig_len != 65) return BCC_SCRIPT_ERR_SCHNORR_SIG_SIZE;
    uint8_t hash_type = 0;  // SIGHASH_DEFAULT
    if (sig_len == 65) {
        hash_type = sig[64];
        if (hash_type == 0) return BCC_SCRIPT_ERR_SCHNORR_SIG_HASHTYPE;
    }
    const int output_type = hash_type == 0 ? 1 : (hash_type & 3);
    if (!(hash_type <= 0x03 || (hash_type >= 0x81 && hash_type <= 0x83)) ||
        (output_type == 3 && n_in >= s.t.vout.size()))
        return BCC_SCRIPT_ERR_SCHNORR_SIG_HASHTYPE;
    TaprootTxJobs& D = J.dev;
    TapJob tj{};
    tj.ttx = tx_record(s, D);
    tj.nin = n_in;
    tj.hash_type = hash_type;
    tj.spend_type = ((tapscript ? 1u : 0u) << 1) + (annex ? 1u : 0u);
    tj.ext_off = (uint32_t)D.ext.size();
    if (annex) {  // sha_annex = SHA256(compactsize(len) || annex)
        scratch.clear();
        put_compact_size(scratch, annex_len);
        scratch.insert(scratch.end(), annex, annex + annex_len);
        D.ext.resize(D.ext.size() + 32);
        sha256(scratch.data(), scratch.size(), &D.ext[D.ext.size() - 32]);
    }
    if (output_type == 3) {  // sha_single_output
        const TxOut& o = s.t.vout[n_in];
        D.ext.resize(D.ext.size() + 32);
        sha256(o.ser.p, o.ser.n, &D.ext[D.ext.size() - 32]);
    }
    if (tapscript) {
        if (leaf_slot) *leaf_slot = (uint32_t)D.ext.size();
        if (leaf32) D.ext.insert(D.ext.end(), leaf32, leaf32 + 32);
        else D.ext.resize(D.ext.size() + 32, 0);
        tj.flags = 1;
        tj.codesep = codesep;
    }
    tj.row = (uint32_t)J.rows();
    D.jobs.push_back(tj);
    J.sig64.insert(J.sig64.end(), sig, sig + 64);
    J.pk32.insert(J.pk32.end(), pk32, pk32 + 32);
    return 0;
}

}  // namespace host
}  // namespace bcc
