/* bcc_amd.h — engine-level C ABI of librbc_amd.so below the drop-in interface.
 *
 * These are the entry points the reference's FFI would bind for the signature hot path once the
 * interpreter defers its checks ("New ABI to add"), plus the device-pointer and
 * workload entry points bench.py drives.  No torch / HIP types appear in any signature: device
 * buffers and streams are passed as plain pointers.
 */
#ifndef BCC_AMD_H
#define BCC_AMD_H

#include <stddef.h>
#include <stdint.h>

#include "bitcoinconsensus.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- tuple level: the deferred CHECKSIG queue flushed to the GPU ---------------------------
 * Replaces the per-signature call CPubKey::Verify -> secp256k1_ecdsa_verify
 * (depend/bitcoin/src/pubkey.cpp:191-207, secp256k1/src/secp256k1.c:423-438).
 * pub65[i] = header byte || x || y (y ignored for 02/03; header 0 marks a key the caller's
 * CPubKey length filter already rejected); msg32 = raw sighash bytes; r32/s32 = big-endian
 * scalars after lax-DER parsing (both zero on overflow).  verdict[i] = 1 iff valid. */
int mi_ecdsa_verify_tuples(const uint8_t* pub65, const uint8_t* msg32, const uint8_t* r32,
                           const uint8_t* s32, uint8_t* verdict, size_t n, int device);

/* Same with all buffers device-resident (separate tag / x / y / r / s / m rows), launched on
 * `stream` (a hipStream_t or NULL).  Asynchronous. */
int mi_ecdsa_verify_device(const uint8_t* d_tag, const uint8_t* d_x, const uint8_t* d_y,
                           const uint8_t* d_r, const uint8_t* d_s, const uint8_t* d_m,
                           uint8_t* d_verdict, size_t n, void* stream);

/* ---- BIP340 Schnorr (config C5) -------------------------------------------------------------
 * Replaces secp256k1_xonly_pubkey_parse + secp256k1_schnorrsig_verify per signature
 * (secp256k1/src/modules/extrakeys/main_impl.h:21-39, modules/schnorrsig/main_impl.h:190-237),
 * as bound by Core's XOnlyPubKey::VerifySchnorr (depend/bitcoin/src/pubkey.cpp:176-182).
 * Row i: sig64 = r.x || s, msg32, xonly32 = the key's 32 serialized bytes (a key that does not
 * parse verifies false).  verdict[i] = 1 iff valid.  Synchronous on `device`; at most
 * bcc_set_host_small_round() rows run on the host CPU and touch no device state, and a device
 * round that fails is handled as "the Taproot side's failure handling" below describes.  Returns
 * 0, or under BCC_DEVICE_FAILURE_ERROR the HIP error of a failed round. */
int mi_schnorr_verify_tuples(const uint8_t* sig64, const uint8_t* msg32, const uint8_t* xonly32,
                             uint8_t* verdict, size_t n, int device);
/* Same with device-resident rows, launched on `stream`.  Asynchronous. */
int mi_schnorr_verify_device(const uint8_t* d_sig64, const uint8_t* d_msg32,
                             const uint8_t* d_xonly32, uint8_t* d_verdict, size_t n,
                             void* stream);

/* ---- BIP341 / BIP342 (Taproot) signature checks ------------------------------------------------
 * Replaces GenericTransactionSignatureChecker::CheckSchnorrSignature per check
 * (depend/bitcoin/src/script/interpreter.cpp:1678-1704): SignatureHashSchnorr (:1491-1574) over
 * the tx's PrecomputedTransactionData initialised with its spent outputs (:1422-1472), then
 * XOnlyPubKey::VerifySchnorr (pubkey.cpp:176-182).  The signature hash (TapSighash tagged
 * SHA-256 and the tx's single-SHA-256 aux hashes) and the BIP340 verification run on the GPU.
 * The fields mirror the checker's inputs: the spending tx, the outputs it spends (one per input,
 * a serialized std::vector<CTxOut> as handed to PrecomputedTransactionData::Init), the input
 * index, the signature (64 bytes, or 65 with the hash_type), the 32-byte x-only key, the
 * sigversion and ScriptExecutionData's annex / tapleaf hash / OP_CODESEPARATOR position.
 * Adjacent items with the same tx and spent_outputs pointers share the per-tx hashes. */
#define BCC_SIGVERSION_TAPROOT 0   /* key path spend (SigVersion::TAPROOT) */
#define BCC_SIGVERSION_TAPSCRIPT 1 /* BIP342 script path (SigVersion::TAPSCRIPT) */
typedef struct bcc_taproot_check {
    const unsigned char* tx;            /* serialized spending tx, exactly tx_len bytes */
    unsigned int tx_len;
    const unsigned char* spent_outputs; /* serialized std::vector<CTxOut>, one per input */
    unsigned int spent_outputs_len;
    unsigned int n_in;
    const unsigned char* sig;           /* 64 or 65 bytes (anything else: SCHNORR_SIG_SIZE) */
    unsigned int sig_len;
    const unsigned char* pubkey32;      /* x-only key bytes */
    int sigversion;                     /* BCC_SIGVERSION_* */
    const unsigned char* annex;         /* the annex witness element incl. 0x50, NULL: none */
    unsigned int annex_len;
    const unsigned char* tapleaf_hash32; /* TAPSCRIPT only (execdata.m_tapleaf_hash); it is what
                                          * bcc_taproot_commit_batch writes to tapleaf_out */
    uint32_t codeseparator_pos;         /* TAPSCRIPT only (0xFFFFFFFF: none executed) */
} bcc_taproot_check;
/* script_error.h:73-75 values written to serror_out */
#define BCC_SCRIPT_ERR_SCHNORR_SIG_SIZE 44
#define BCC_SCRIPT_ERR_SCHNORR_SIG_HASHTYPE 45
#define BCC_SCRIPT_ERR_SCHNORR_SIG 46
/* ret_out[i] = 1 (valid) or 0 (serror_out[i] = one of the three codes above), or -1 where the
 * reference checker cannot be built and asserts instead: the tx does not deserialize to exactly
 * tx_len bytes, the spent outputs do not parse or their count differs from the tx's inputs,
 * n_in >= inputs, or no witness-bearing input spends a 34-byte OP_1 script (the tx data would not
 * be BIP341-ready); serror_out[i] = 1 (SCRIPT_ERR_UNKNOWN_ERROR) then.  sighash_out (optional,
 * 32 bytes per item): the signature hash where one was computed, else zeros.  Synchronous on
 * `device`, or for device = -1 spread over the bcc_set_devices() GPUs; a round of at most
 * bcc_set_host_small_round() checks runs on the host CPU.  Returns 0, or -1 on bad arguments, or
 * -1 on a device failure under BCC_DEVICE_FAILURE_ERROR (then no output is meaningful; under the
 * default policy the failed round is verified on the host and the call returns its exact result:
 * "the Taproot side's failure handling" below). */
int bcc_taproot_verify_batch(const bcc_taproot_check* items, size_t n, int* ret_out,
                             int* serror_out, unsigned char* sighash_out, int device);

/* ---- BIP341 script-path commitment ---------------------------------------------------------------
 * Replaces the commitment check of a script-path spend in VerifyWitnessProgram
 * (depend/bitcoin/src/script/interpreter.cpp:1909-1914): the control-size rule, then
 * VerifyTaprootCommitment (:1834-1853) = the TapLeaf hash of the script, one TapBranch hash per
 * 32-byte node of the control block, the TapTweak hash and XOnlyPubKey::CheckPayToContract
 * (pubkey.cpp:184-189): lift_x(p) + t G == (q, parity).  All hashes and the curve check run on the
 * GPU.  The caller has removed the annex; any leaf version is accepted (leaf version =
 * control[0] & 0xfe, parity = control[0] & 1, p = control[1..33)). */
typedef struct bcc_taproot_commit {
    const unsigned char* control;   /* the control block witness element */
    unsigned int control_len;
    const unsigned char* script;    /* the leaf script (may be empty; NULL only with script_len 0) */
    unsigned int script_len;
    const unsigned char* program32; /* the 32-byte v1 witness program q */
} bcc_taproot_commit;
/* script_error.h values written to serror_out */
#define BCC_SCRIPT_ERR_WITNESS_PROGRAM_MISMATCH 39
#define BCC_SCRIPT_ERR_TAPROOT_WRONG_CONTROL_SIZE 47
/* Per item: ret_out[i] = 1, serror_out[i] = 0 when the commitment holds; ret 0 / serror 47 when
 * control_len < 33, control_len > 33 + 32 * 128 or (control_len - 33) % 32 != 0 (nothing is hashed
 * for such an item); ret 0 / serror 39 when VerifyTaprootCommitment is false.  tapleaf_out
 * (optional, 32 bytes per item): the TapLeaf hash of every item whose control size is valid,
 * whether or not the commitment holds, else zeros; a caller hands it on as
 * bcc_taproot_check.tapleaf_hash32.  Synchronous on `device`, or for device = -1 spread in
 * contiguous ranges over the bcc_set_devices() GPUs; batches of at most
 * bcc_set_host_small_round() items run the same lane code on the host.  Results never depend on
 * the device set, the round cut or the thread count.  Returns 0 (also for n == 0), or -1 for null
 * arrays, an item with a null control, program32 or (with script_len > 0) script: nothing is
 * verified then; or -1 on a device failure under BCC_DEVICE_FAILURE_ERROR (then no output is
 * meaningful; under the default policy the failed round runs the same lane code on the host). */
int bcc_taproot_commit_batch(const bcc_taproot_commit* items, size_t n, int* ret_out,
                             int* serror_out, unsigned char* tapleaf_out, int device);

/* ---- whole Taproot inputs --------------------------------------------------------------------
 * Replaces VerifyScript (depend/bitcoin/src/script/interpreter.cpp:1937-2056) for an input that
 * spends a native v1 witness program: VerifyWitnessProgram's v1 branch (:1889-1927) with the annex
 * rule, the key path, the control-size rule, the commitment, the leaf version, and for leaf version
 * 0xc0 the tapscript (ExecuteWitnessScript / EvalScript with SigVersion::TAPSCRIPT, :1794-1832,
 * :431-1259, EvalChecksigTapscript :371-429).  The host interprets each tapscript once: a BIP342
 * signature opcode with a non-empty signature either verifies or fails the whole script, so the
 * pass assumes it verifies and queues the check.  A round's commitments (TapLeaf / TapBranch /
 * TapTweak hashes, the curve check) and all its signature checks (key path and queued tapscript
 * checks: SigMsg, TapSighash, BIP340) then run on the GPU in one stream; the TapLeaf hash reaches
 * the signature hashes on the device. */
typedef struct bcc_taproot_spend {
    const unsigned char* tx;            /* serialized spending tx, exactly tx_len bytes */
    unsigned int tx_len;
    const unsigned char* spent_outputs; /* serialized std::vector<CTxOut>, one per input */
    unsigned int spent_outputs_len;
    unsigned int n_in;
} bcc_taproot_spend;
/* script_error.h values this entry adds to the ones above */
#define BCC_SCRIPT_ERR_EVAL_FALSE 2
#define BCC_SCRIPT_ERR_PUSH_SIZE 5
#define BCC_SCRIPT_ERR_STACK_SIZE 7
#define BCC_SCRIPT_ERR_BAD_OPCODE 15
#define BCC_SCRIPT_ERR_PUBKEYTYPE 28
#define BCC_SCRIPT_ERR_CLEANSTACK 29
#define BCC_SCRIPT_ERR_WITNESS_PROGRAM_WITNESS_EMPTY 38
#define BCC_SCRIPT_ERR_WITNESS_MALLEATED 40
#define BCC_SCRIPT_ERR_TAPSCRIPT_VALIDATION_WEIGHT 48
#define BCC_SCRIPT_ERR_TAPSCRIPT_CHECKMULTISIG 49
#define BCC_SCRIPT_ERR_TAPSCRIPT_MINIMALIF 50
/* Per item, ret_out[i] / serror_out[i] are what VerifyScript(tx.vin[n_in].scriptSig,
 * spent_outputs[n_in].scriptPubKey, &witness, flags, checker, &serror) returns and writes, with
 * flags = P2SH | DERSIG | NULLDUMMY | CHECKLOCKTIMEVERIFY | CHECKSEQUENCEVERIFY | WITNESS | TAPROOT
 * (0xE15 | 1 << 17) and the checker's PrecomputedTransactionData initialised with the spent
 * outputs: 1 / 0 when the input verifies, else 0 and the script_error.h number (any ScriptError the
 * interpreter can set, not only the ones defined here).  A spend's result is, in this order: the
 * control-size error; the commitment mismatch; SCHNORR_SIG when a queued signature check fails;
 * the interpreter's own result.  ret -1 / serror 1 where the reference checker cannot be built
 * (of the conditions bcc_taproot_verify_batch documents: the tx does not deserialize to exactly
 * tx_len bytes, the spent outputs do not parse or their count differs from the tx's inputs,
 * n_in >= inputs; BIP341-readiness follows from the next condition whenever a signature check is
 * reached), where the spent scriptPubKey is not exactly OP_1 0x20 <32 bytes> (this entry is for
 * native v1 programs; everything else belongs to bitcoinconsensus_verify_batch), and where the
 * result of a non-empty scriptSig depends on ECDSA checks of non-empty signatures, for which this
 * entry has no lane: a scriptSig without such a check gives its own error or WITNESS_MALLEATED; one
 * that meets exactly one is run with both verdicts and reported when both runs agree (a lone
 * OP_CHECKSIG only pushes its verdict: WITNESS_MALLEATED either way); any other gets ret -1.
 * Synchronous on `device`, or for device = -1 spread in contiguous ranges over the
 * bcc_set_devices() GPUs; a round of at most bcc_set_host_small_round() checks (signature checks
 * plus commitments) runs on the host CPU altogether: the commitment lane code and the kernels'
 * BIP340 lane, with no device state touched.  Adjacent items with the same tx and spent_outputs
 * pointers share the per-tx work.  Results never depend on the device set, the round cut, the
 * thread count or bcc_set_host_small_round.  Returns 0 (also for n == 0), -1 for null arrays or an
 * item with a null tx or spent_outputs (nothing is verified then), or -1 on a device failure under
 * BCC_DEVICE_FAILURE_ERROR (then no output is meaningful).
 *
 * The Taproot side's failure handling (this entry, bcc_taproot_verify_batch,
 * bcc_taproot_commit_batch, mi_schnorr_verify_tuples, mi_xonly_tweak_check_tuples, and through
 * them bcc_verify_inputs_batch / bcc_verify_input) is bitcoinconsensus_verify_batch's: a device
 * round that fails with a transient HIP error (out of memory, not ready, a staging limit) is
 * re-run once on a fresh context; if it fails again, or the error leaves the context unusable,
 * bcc_set_device_failure_policy decides.  Under BCC_DEVICE_FAILURE_HOST (the default) the round is
 * rebuilt from its items and verified on the host CPU by the engine's own code (host SHA-256 over
 * the very job records the kernels read, the kernels' BIP340 and commitment lanes over the host
 * comb), logged on stderr and counted by bcc_host_fallback_rounds; after an error that leaves the
 * context unusable the call's remaining rounds on that device go the same way without another
 * launch, and the entry returns its exact result.  Under BCC_DEVICE_FAILURE_ERROR the entry
 * returns its error.  bcc_debug_fail_device_rounds reaches every one of these rounds, before it
 * is launched. */
int bcc_taproot_spend_batch(const bcc_taproot_spend* items, size_t n, int* ret_out,
                            int* serror_out, int device);
/* Items per device round of bcc_taproot_spend_batch (0, the default: the engine's choice, 65,536).
 * Rounds rotate over the Taproot contexts, so one round's upload runs beside the previous round's
 * kernels.  For tests: a small value puts round boundaries inside a small batch.  Returns 0. */
int bcc_set_spend_round(size_t items);

/* ---- any input against its spent outputs ------------------------------------------------------
 * The block validator's one call: VerifyScript (depend/bitcoin/src/script/interpreter.cpp:
 * 1937-2056) for input n_in of a transaction given the outputs the whole transaction spends, as
 * later libconsensus versions take them (a serialized std::vector<CTxOut>, one per input: what
 * PrecomputedTransactionData::Init receives, :1422-1472).  The scriptPubKey and the amount are read
 * from spent_outputs[n_in].  Inputs that spend a native v1 program go to the engine of
 * bcc_taproot_spend_batch, every other input to the engine of bitcoinconsensus_verify_batch, in one
 * stable partition (adjacent items with the same tx and spent_outputs pointers keep sharing their
 * per-tx work on either side); both run as they do under their own entry points.
 * The item is bcc_taproot_spend's: tx, tx_len, spent_outputs, spent_outputs_len, n_in. */
#define BCC_SCRIPT_FLAGS_VERIFY_TAPROOT (1U << 17) /* SCRIPT_VERIFY_TAPROOT (interpreter.h) */
#define BCC_ERR_SPENT_OUTPUTS_MISMATCH 7           /* (6 is BCC_ERR_DEVICE_FAILURE) */
typedef bcc_taproot_spend bcc_input;
/* Per item, ret_out[i] / err_out[i] (err_out may be NULL) are decided by the first rule that
 * applies:
 *  1. flags.  Accepted: any subset of bitcoinconsensus_SCRIPT_FLAGS_VERIFY_ALL, or exactly
 *     VERIFY_ALL | BCC_SCRIPT_FLAGS_VERIFY_TAPROOT (the tapscript interpreter and the Taproot
 *     kernels stand for that one set, every block's since activation).  Anything else (TAPROOT with
 *     an incomplete base set, any other bit): ret 0 / bitcoinconsensus_ERR_INVALID_FLAGS for every
 *     item.
 *  2. the transaction.  ret 0 / the error bitcoinconsensus_verify_script_with_amount writes for
 *     this tx, tx_len and n_in whatever the script: ERR_TX_DESERIALIZE, ERR_TX_INDEX,
 *     ERR_TX_SIZE_MISMATCH, in that order (bitcoinconsensus.cpp:79-102).
 *  3. the spent outputs.  They must deserialize as a std::vector<CTxOut> with no byte left over and
 *     hold as many outputs as the tx has inputs, else ret 0 / BCC_ERR_SPENT_OUTPUTS_MISMATCH, also
 *     for an input whose own check would not read the other outputs.
 *  4. the script.  err OK, and ret = VerifyScript(tx.vin[n_in].scriptSig,
 *     spent_outputs[n_in].scriptPubKey, &witness, flags, checker) with the checker's amount
 *     spent_outputs[n_in].nValue and its PrecomputedTransactionData initialised with the spent
 *     outputs.  The script error is not reported (bcc_taproot_spend_batch reports it for v1
 *     inputs).  Without TAPROOT a native v1 program passes unchecked, as in
 *     bitcoinconsensus_verify_batch.  A v1 input for which bcc_taproot_spend_batch answers ret -1
 *     after rules 1-3 (a non-empty scriptSig that meets ECDSA checks) is invalid under every
 *     verdict: ret 0 / err OK.
 * Returns the number of valid items (0 for n == 0), or -1 for a null items or ret_out or an item
 * with a null tx or spent_outputs (nothing is verified then), or -1 when a device round failed:
 * the non-v1 side follows bcc_set_device_failure_policy exactly as bitcoinconsensus_verify_batch
 * does (its unfinished items carry BCC_ERR_DEVICE_FAILURE), and so does the v1 side: under
 * BCC_DEVICE_FAILURE_HOST a failed round of either side is verified on the host and the call
 * returns its exact result; under BCC_DEVICE_FAILURE_ERROR the items a failed round of either side
 * left without a verdict get ret 0 / BCC_ERR_DEVICE_FAILURE while every other item keeps its
 * result.  Both sides use the devices of bcc_set_device /
 * bcc_set_devices.  Results never depend on the device set, bcc_set_pipeline_chunk,
 * bcc_set_spend_round or the thread count.  Synchronous.  A call with items for both sides runs them
 * at the same time: the non-v1 subset on the calling thread, the v1 subset on a second thread that
 * the calling thread keeps as its own concurrent caller (its team and device state are released by
 * the calling thread's bcc_release_thread_state, and it is joined when the calling thread exits). */
long bcc_verify_inputs_batch(const bcc_input* items, size_t n, unsigned int flags, int* ret_out,
                             int* err_out);
/* One input: ret, and *err when err != NULL.  A null tx or spent_outputs counts as an empty buffer.
 * A lone input is a small round (bcc_set_host_small_round): it is verified on the host CPU and opens
 * no device.  Where the batch call would return -1 for a failed device round (only under
 * BCC_DEVICE_FAILURE_ERROR: the default policy verifies such a round on the host) there is no
 * verdict, and the call aborts as bitcoinconsensus_verify_script_with_amount does. */
int bcc_verify_input(const unsigned char* tx, unsigned int tx_len,
                     const unsigned char* spent_outputs, unsigned int spent_outputs_len,
                     unsigned int n_in, unsigned int flags, int* err);
typedef struct bcc_inputs_stats {
    /* items = ecdsa_side_items + taproot_side_items + host_decided_items (rules 1-3) */
    size_t items, ecdsa_side_items, taproot_side_items, host_decided_items;
    /* the routing pass (rules 1-3, locating spent[n_in], the partition), each side's call (the two
     * overlap when both sides have items, so they do not add up to the total), the whole call */
    double route_seconds, ecdsa_side_seconds, taproot_side_seconds, total_seconds;
} bcc_inputs_stats;
/* Statistics of the calling thread's last bcc_verify_inputs_batch / bcc_verify_input call. */
void bcc_last_inputs_stats(bcc_inputs_stats* out);

/* ---- a block's transaction hashes and merkle commitments ---------------------------------------
 * What a validator hashes around bcc_verify_inputs_batch: every transaction's txid (it names the
 * spent outputs) and wtxid (primitives/transaction.cpp:67-83), the header's merkle root with the
 * CVE-2012-2459 mutation test (consensus/merkle.cpp:45-84, validation.cpp:3364-3380) and the
 * segwit coinbase commitment (validation.cpp:3575-3610, consensus/validation.h:161-179).
 * All 32-byte hashes are raw digest bytes (uint256::begin() order): the order of a prevout's txid
 * field and of the header's merkle field, not the reversed hex display.
 *
 * Conventions of the three entries: synchronous on `device`; -1 spreads whole blocks or contiguous
 * item ranges over the bcc_set_devices() GPUs (bcc_merkle_root: one tree, the first of them).  They
 * return 0, or -1 for null arrays or null item buffers (nothing is computed then), or -1 on a
 * device failure under BCC_DEVICE_FAILURE_ERROR (then no output is meaningful).  A device round is
 * the transactions of some whole blocks (bcc_tx_hashes_batch: of an item range), uploaded once with
 * their witnesses, one SHA-256 lane per digest, then one launch per merkle level over every tree
 * of the round.  Transactions whose digests need more than bcc_set_host_txhash_blocks() 64-byte
 * blocks are hashed on the host while the kernel runs: a lane is one serial chain.  A round of at
 * most the entries' small-round threshold of transactions (leaves), and a round the device could
 * not deliver after one retry, is evaluated by the host over the same records; the threshold is the
 * engine's own (2,048, provisional) unless bcc_set_host_small_round() is larger, and
 * bcc_set_host_small_round(0) turns it off like every other.  The failure rules
 * are the Taproot side's (above), bcc_debug_fail_device_rounds[_code] reaches these rounds too.
 * Results never depend on the device set, the round cut, the thread count or any threshold. */
typedef struct bcc_tx_ref { const unsigned char* tx; unsigned int tx_len; } bcc_tx_ref;
/* txid_out / wtxid_out: 32 bytes per item, either may be NULL.  err_out[i]: 0, or
 * bitcoinconsensus_ERR_TX_DESERIALIZE / ERR_TX_SIZE_MISMATCH by the rules of
 * bitcoinconsensus.cpp:79-102 (hashes zero then).  txid = SHA-256d of the serialization without
 * marker, flag and witnesses; wtxid = SHA-256d of all tx_len bytes (equal to txid for a tx
 * without witness data). */
int bcc_tx_hashes_batch(const bcc_tx_ref* items, size_t n, unsigned char* txid_out,
                        unsigned char* wtxid_out, int* err_out, int device);

/* ComputeMerkleRoot (consensus/merkle.cpp:45-62): n == 0 gives the zero hash; *mutated (may be
 * NULL) as the reference sets it. */
int bcc_merkle_root(const unsigned char* leaves32, size_t n, unsigned char* root32,
                    int* mutated, int device);

typedef struct bcc_block_ref {
    const unsigned char* block; size_t block_len;   /* 80-byte header, CompactSize count, txs;
                                                       a buffer of 2^31 bytes or more does not
                                                       deserialize */
    int segwit_active;                              /* nHeight >= SegwitHeight */
    unsigned char* txid_out; size_t txid_cap;       /* optional: n_tx * 32 bytes are written when
                                                       txid_cap >= n_tx, else none */
} bcc_block_ref;
typedef struct bcc_block_result {
    int status;              /* BCC_BLOCK_* below: the first rule that applies */
    unsigned int n_tx;
    int commit_pos;          /* GetWitnessCommitmentIndex, -1: none */
    unsigned char merkle_root[32], witness_root[32];  /* witness_root zero unless computed */
} bcc_block_result;
#define BCC_BLOCK_OK 0
#define BCC_BLOCK_ERR_DESERIALIZE 1        /* short header, bad count, a tx that does not parse,
                                              bytes left over */
#define BCC_BLOCK_ERR_EMPTY 2              /* no transactions */
#define BCC_BLOCK_ERR_MERKLE_ROOT 3        /* "bad-txnmrklroot" */
#define BCC_BLOCK_ERR_DUPLICATE 4          /* "bad-txns-duplicate" (mutated) */
#define BCC_BLOCK_ERR_WITNESS_NONCE_SIZE 5 /* "bad-witness-nonce-size" */
#define BCC_BLOCK_ERR_WITNESS_MERKLE 6     /* "bad-witness-merkle-match" */
#define BCC_BLOCK_ERR_UNEXPECTED_WITNESS 7 /* "unexpected-witness" */
/* Per block, in the order Core applies the rules: the header root against header[36..68); the
 * mutation flag; then, with segwit_active and a commitment output, the reserved value's shape
 * (coinbase input 0's witness is exactly one 32-byte element) and SHA-256d(witness root ||
 * reserved value) against scriptPubKey[6..38) of the last commitment output (the witness tree's
 * own mutation flag is ignored); otherwise any transaction with witness data gives
 * UNEXPECTED_WITNESS.  The engine's own rule: a coinbase with no inputs on a path that would read
 * vin[0] gives WITNESS_NONCE_SIZE (Core rejects such a block earlier, "bad-txns-vin-empty").
 * The witness tree is computed only for a block that reaches the commitment comparison.  A block
 * that does not deserialize or is empty has n_tx 0, commit_pos -1 and zero roots. */
int bcc_block_commitments_batch(const bcc_block_ref* blocks, size_t n, bcc_block_result* out,
                                int device);
typedef struct bcc_block_stats {
    size_t blocks, txs;          /* blocks (trees for bcc_merkle_root) and transactions (leaves) */
    size_t bytes_hashed;         /* message bytes of every SHA-256d: digests, 64 per tree node */
    size_t device_rounds, host_rounds;  /* host_rounds: small rounds + failure fallbacks */
    size_t host_long_txs;        /* transactions of device rounds hashed on the host */
    size_t merkle_launches;      /* merkle level launches of the device rounds */
    size_t device_retries;
} bcc_block_stats;
/* Statistics of the calling thread's last call of one of the three entries. */
void bcc_last_block_stats(bcc_block_stats* out);
/* Transactions per device round (0, the default: the engine's choice, 262,144; a block is never
 * split).  For tests: a small value puts round cuts inside a small batch.  Returns 0. */
int bcc_set_block_round(size_t txs);
/* The long-chain threshold in 64-byte SHA-256 blocks (0: no transaction goes to the host).
 * Returns 0. */
int bcc_set_host_txhash_blocks(unsigned blocks);
/* Where the calling thread's last call on one device spent its time, in milliseconds, summed over
 * its device rounds.  Event times: ms6[0] the transaction hashing kernel, ms6[1] the merkle level
 * launches, ms6[2] the uploads, ms6[3] the downloads; zeros unless BCC_BLOCK_TIMING=1 was in the
 * environment when the library was loaded (the events cost a few microseconds each).  Host clocks:
 * ms6[4] parsing the blocks or transactions, ms6[5] staging a round (records, tables, the
 * page-locked image of the upload).  For tools/block_bench.py. */
void bcc_block_last_timing_ms(double* ms6);

/* ---- a block's transaction rules, sigops, finality, coinbase height and sizes ---------------------
 * The rest of CheckBlock and ContextualCheckBlock (validation.cpp:3387-3416, 3543-3620) that needs
 * no UTXO: CheckTransaction for every transaction (consensus/tx_check.cpp:10-58, the duplicate-input
 * rule included), GetLegacySigOpCount and IsFinalTx (consensus/tx_verify.cpp:17-28, 107-119), the
 * coinbase position, the BIP34 height prefix, the stripped size and the weight.  The transactions
 * are the ones a block round has uploaded for hashing: one lane per transaction walks its inputs and
 * outputs, one lane per input of a transaction with two or more inputs probes a hash table of
 * outpoints, one wave per block reduces the records; one record per block comes back.  The
 * conventions are the block entries' above (synchronous, device == -1, null arguments, the host
 * route for small rounds, long transactions and device failures, results independent of every
 * setting); bcc_last_block_stats and bcc_block_last_timing_ms describe these entries too.
 *
 * Out of scope, the caller's: the UTXO-dependent rules (CheckTxInputs, P2SH and witness sigop cost,
 * BIP68, BIP30, a double spend between two transactions of a block), and deciding the lock-time
 * cutoff and the activation flags. */
#define BCC_TX_OK 0
#define BCC_TX_ERR_VIN_EMPTY 16            /* "bad-txns-vin-empty" */
#define BCC_TX_ERR_VOUT_EMPTY 17           /* "bad-txns-vout-empty" */
#define BCC_TX_ERR_OVERSIZE 18             /* "bad-txns-oversize": stripped size * 4 > 4,000,000 */
#define BCC_TX_ERR_VOUT_NEGATIVE 19        /* "bad-txns-vout-negative" */
#define BCC_TX_ERR_VOUT_TOOLARGE 20        /* "bad-txns-vout-toolarge" */
#define BCC_TX_ERR_TXOUTTOTAL_TOOLARGE 21  /* "bad-txns-txouttotal-toolarge" */
#define BCC_TX_ERR_INPUTS_DUPLICATE 22     /* "bad-txns-inputs-duplicate" (CVE-2018-17144) */
#define BCC_TX_ERR_CB_LENGTH 23            /* "bad-cb-length" */
#define BCC_TX_ERR_PREVOUT_NULL 24         /* "bad-txns-prevout-null" */
typedef struct bcc_tx_check_result {
    int status;                  /* BCC_TX_OK, a BCC_TX_ERR_* above (the first in CheckTransaction's
                                    order), or bitcoinconsensus_ERR_TX_DESERIALIZE /
                                    ERR_TX_SIZE_MISMATCH as bcc_tx_hashes_batch's err (the other
                                    fields are zero then) */
    unsigned int n_in, n_out, sigops, lock_time;   /* sigops: GetLegacySigOpCount, unscaled */
    unsigned int stripped_size, total_size;        /* weight = 3 * stripped + total */
    unsigned char is_coinbase, all_final;          /* all_final: every nSequence is 0xffffffff */
} bcc_tx_check_result;
int bcc_tx_check_batch(const bcc_tx_ref* items, size_t n, bcc_tx_check_result* out, int device);

/* (enumerators, not macros: the BCC_BLOCK_* macros above are the commitments entry's eight) */
enum { BCC_BLOCK_SEGWIT_ACTIVE = 1, BCC_BLOCK_BIP34_ACTIVE = 2 };
typedef struct bcc_block_check_ref {
    const unsigned char* block; size_t block_len;
    int height;                  /* of this block */
    int64_t lock_time_cutoff;    /* the caller's choice: the median time past of the previous block
                                    (BIP113) or the block's own time */
    unsigned int flags;          /* BCC_BLOCK_SEGWIT_ACTIVE | BCC_BLOCK_BIP34_ACTIVE */
} bcc_block_check_ref;
typedef struct bcc_block_check_result {
    int status;                  /* BCC_BLOCK_*: the first rule that applies, in the order below */
    int tx_index;                /* the transaction BCC_BLOCK_ERR_TX or ERR_NONFINAL names, else -1 */
    int tx_status;               /* with BCC_BLOCK_ERR_TX: that transaction's BCC_TX_ERR_*; else 0 */
    unsigned int n_tx;
    int commit_pos;
    uint64_t sigops;             /* the sum of GetLegacySigOpCount, unscaled */
    uint64_t stripped_size;      /* the block without witness data: 80 + the count + the transactions */
    uint64_t weight;             /* 3 * stripped_size + block_len */
    unsigned char merkle_root[32], witness_root[32];
} bcc_block_check_result;
enum {                                 /* the statuses continue BCC_BLOCK_* above */
    BCC_BLOCK_ERR_LENGTH = 8,          /* "bad-blk-length" */
    BCC_BLOCK_ERR_CB_MISSING = 9,      /* "bad-cb-missing" */
    BCC_BLOCK_ERR_CB_MULTIPLE = 10,    /* "bad-cb-multiple" */
    BCC_BLOCK_ERR_TX = 11,             /* CheckTransaction refused tx_index with tx_status */
    BCC_BLOCK_ERR_SIGOPS = 12,         /* "bad-blk-sigops" */
    BCC_BLOCK_ERR_NONFINAL = 13,       /* "bad-txns-nonfinal" */
    BCC_BLOCK_ERR_CB_HEIGHT = 14,      /* "bad-cb-height" */
    BCC_BLOCK_ERR_WEIGHT = 15          /* "bad-blk-weight" */
};
/* Per block, Core's order (CheckBlock, then ContextualCheckBlock): deserialize; empty; the merkle
 * root; the mutation flag; length (n_tx * 4 > 4,000,000 or stripped_size * 4 > 4,000,000); a first
 * transaction that is no coinbase; a later one that is; the first transaction, in block order, that
 * CheckTransaction refuses; sigops * 4 > 80,000; the first transaction that is not final at
 * (height, lock_time_cutoff); with BCC_BLOCK_BIP34_ACTIVE the coinbase scriptSig not starting with
 * CScript() << height; the three witness-commitment statuses as bcc_block_commitments_batch decides
 * them; weight > 4,000,000.  n_tx, commit_pos and the roots are that entry's on the same bytes; the
 * sums are filled for every block with transactions.  One upload serves the hashes and the rules. */
int bcc_block_check_batch(const bcc_block_check_ref* blocks, size_t n, bcc_block_check_result* out,
                          int device);
/* Where the rules' part of the calling thread's last call on one device spent its time, in
 * milliseconds, summed over its device rounds.  Event times: ms5[0] the transaction lanes, ms5[1]
 * the duplicate-input lanes, ms5[2] the block lanes (zeros unless BCC_BLOCK_TIMING=1 was in the
 * environment when the library was loaded).  Host clocks: ms5[3] planning the rounds' rule records,
 * ms5[4] the long transactions the host evaluated. */
void bcc_block_rules_last_timing_ms(double* ms5);
/* For tests: the slot of a table of 2^log2_slots words (1 <= log2_slots <= 31) where the input with
 * these 36 outpoint bytes in the transaction at row tx_row of its round starts probing, and the
 * log2_slots a round with `rows` input rows uses (rows: the inputs of its transactions with two or
 * more inputs). */
unsigned int bcc_debug_outpoint_slot(unsigned int tx_row, const unsigned char* outpoint36,
                                     unsigned int log2_slots);
unsigned int bcc_debug_dup_table_log2(size_t rows);

/* ---- header chains: block hashes, proof of work, retargets ----------------------------------------
 * What CheckBlockHeader and ContextualCheckBlockHeader decide for a run of consecutive 80-byte
 * headers (validation.cpp:3341-3350, 3496-3535): the block hash (SHA-256d of the header),
 * CheckProofOfWork (pow.cpp:74-91), the link to the header before, the expected nBits
 * (GetNextWorkRequired / CalculateNextWorkRequired, pow.cpp:13-72, arith_uint256.cpp:203-244), the
 * median time past of the 11 blocks before (chain.h:257-275), the caller's upper time bound and the
 * three version gates; and the chain's work (GetBlockProof, chain.cpp:122-135).  Hashes are raw
 * digest bytes, as in the block entries above.  One SHA-256d lane per header, then one context lane
 * per header, on the GPU. */
typedef struct bcc_header_params {          /* Consensus::Params, the fields the header rules read */
    unsigned char pow_limit[32];            /* uint256 bytes, as uint256::begin() orders them */
    int64_t pow_target_timespan, pow_target_spacing; /* both > 0, interval = timespan / spacing >= 1,
                                               timespan < 2^30 (the retarget's factors are 32-bit) */
    int pow_no_retargeting;                 /* fPowNoRetargeting */
    int pow_allow_min_difficulty;           /* must be 0: the testnet exception is not implemented */
    int bip34_height, bip66_height, bip65_height;
} bcc_header_params;
typedef struct bcc_header_anchor {          /* the block headers[0] builds on */
    int height;                             /* >= 0; headers[0] has height + 1 */
    unsigned char hash[32];
    uint32_t bits;
    uint32_t times[11]; unsigned n_times;   /* nTime of the anchor and its ancestors, newest first:
                                               min(11, height + 1) of them, at least the anchor's */
    uint32_t period_first_time;             /* nTime of the first block of the retarget period the
                                               next boundary closes (the block `interval` below that
                                               boundary, which may be the anchor itself); ignored
                                               with pow_no_retargeting */
} bcc_header_anchor;
#define BCC_HEADER_OK 0
#define BCC_HEADER_HIGH_HASH 1        /* CheckProofOfWork false: "high-hash" */
#define BCC_HEADER_PREV_MISMATCH 2    /* hashPrevBlock != hash of the header before it / the anchor */
#define BCC_HEADER_BAD_DIFFBITS 3     /* "bad-diffbits" */
#define BCC_HEADER_TIME_TOO_OLD 4     /* nTime <= median time past of the 11 before it */
#define BCC_HEADER_TIME_TOO_NEW 5     /* nTime > max_time; max_time 0: rule off */
#define BCC_HEADER_BAD_VERSION 6      /* "bad-version" */
/* status_out[i] (required): the first rule header i breaks, in the order above.  Header i is judged
 * against the header bytes before it as given, whether or not those headers passed.  anchor NULL:
 * headers[0] is a genesis of height 0 and gets the proof-of-work rule only.  nTime is widened
 * unsigned, nVersion is signed.  hash_out (optional, 32 bytes per header): every header's hash.
 * chain_work_out (optional): the sum of GetBlockProof over the headers before the first one whose
 * status is not OK, as a little-endian 256-bit number; the anchor's work is not in it.  Returns the
 * index of that first header, n when every status is OK (0 for n == 0), or -1: a null headers80,
 * params or status_out, parameters outside the ranges above, an anchor with a negative height or
 * n_times outside 1..11, heights past 2^31 - 1, or a device failure under BCC_DEVICE_FAILURE_ERROR
 * (no output is meaningful then).  Synchronous on `device`; -1 spreads contiguous ranges over the
 * bcc_set_devices() GPUs.  A round is at most bcc_set_header_round() headers, uploaded in one copy
 * with what its first headers need from before it (the last hash and bits, eleven times, the
 * period's first time), which the host reads from the header bytes themselves.  Rounds of at most
 * the entry's small-round threshold (128 headers, measured: DESIGN.md 3.18), and rounds the device
 * could not deliver after one retry, run the same lane code on the host;
 * bcc_set_host_small_round() and the failure rules apply as they do to the block entries, and
 * bcc_debug_fail_device_rounds[_code] reaches these rounds too.  Results never depend on the device
 * set, the round cut, the thread count or any threshold. */
long bcc_headers_batch(const unsigned char* headers80, size_t n, const bcc_header_params* params,
                       const bcc_header_anchor* anchor, int64_t max_time, unsigned char* hash_out,
                       int* status_out, unsigned char* chain_work_out, int device);
/* The layer below: ok_out[i] = CheckProofOfWork(hash32_i, bits[i]) under pow_limit (32 uint256
 * bytes), one lane per row.  Returns 0 (also for n == 0), -1 for null arrays, or the HIP error of a
 * failed round under BCC_DEVICE_FAILURE_ERROR.  device -1: the first of the bcc_set_devices() GPUs.
 * Its small-round threshold is 2,048 rows (provisional: not measured). */
int mi_pow_check_tuples(const unsigned char* hash32, const uint32_t* bits, size_t n,
                        const unsigned char* pow_limit, unsigned char* ok_out, int device);
typedef struct bcc_header_stats {
    size_t headers;                     /* headers (rows of mi_pow_check_tuples) */
    size_t device_rounds, host_rounds;  /* host_rounds: small rounds + failure fallbacks */
    size_t device_retries;
} bcc_header_stats;
/* Statistics of the calling thread's last bcc_headers_batch / mi_pow_check_tuples call. */
void bcc_last_header_stats(bcc_header_stats* out);
/* Headers per device round (0, the default: the engine's choice, 262,144).  For tests: a small value
 * puts round cuts inside a small batch.  Returns 0. */
int bcc_set_header_round(size_t headers);
/* Event times in milliseconds of the calling thread's last bcc_headers_batch call on one device,
 * summed over its rounds: ms4[0] header_hash_kernel, ms4[1] header_context_kernel, ms4[2] the
 * uploads, ms4[3] the downloads.  Zeros unless BCC_HEADER_TIMING=1 was in the environment when the
 * library was loaded.  For tools/headers_bench.py. */
void bcc_header_last_timing_ms(double* ms4);

/* Where the Taproot side's work ran. */
typedef struct bcc_taproot_stats {
    size_t items, checks, commits;   /* signature rows and commitment lanes of the call */
    size_t rounds, host_rounds;      /* host_rounds: small rounds + failure fallbacks   */
    size_t host_checks;              /* rows + commitments the host verified            */
    size_t device_retries;
} bcc_taproot_stats;
/* Statistics of the calling thread's last Taproot-side call: bcc_taproot_verify_batch,
 * bcc_taproot_spend_batch, bcc_taproot_commit_batch, mi_schnorr_verify_tuples,
 * mi_xonly_tweak_check_tuples, or the v1 side of bcc_verify_inputs_batch / bcc_verify_input (a
 * call without v1 items leaves them as they were). */
void bcc_last_taproot_stats(bcc_taproot_stats* out);

/* The layer below (the role mi_schnorr_verify_tuples has for signatures): n rows of the tweaked
 * key q, the parity byte, the internal key p and the tweak t (32-byte big-endian strings).
 * verdict[i] = 1 iff secp256k1_xonly_pubkey_parse(internal32_i) succeeds and
 * secp256k1_xonly_pubkey_tweak_add_check(tweaked32_i, parity_i, ., tweak32_i) returns 1
 * (secp256k1/src/modules/extrakeys/main_impl.h:21-41, 109-129); a parity byte other than 0 or 1
 * gives 0.  Synchronous on `device` (-1: spread over the bcc_set_devices() GPUs); at most
 * bcc_set_host_small_round() rows run on the host.  Returns 0, -1 for null arrays, or a HIP error
 * code on a device failure under BCC_DEVICE_FAILURE_ERROR (the default policy runs a failed
 * round's rows through the same lane code on the host). */
int mi_xonly_tweak_check_tuples(const uint8_t* tweaked32, const uint8_t* parity,
                                const uint8_t* internal32, const uint8_t* tweak32,
                                uint8_t* verdict, size_t n, int device);

/* Event times in milliseconds of the commitment kernels during the calling thread's last
 * bcc_taproot_commit_batch / mi_xonly_tweak_check_tuples call on one device, summed over its
 * rounds: ms3[0] the hashing kernel, ms3[1] the curve kernel (lift, comb, addition), ms3[2] the
 * batched inversion and comparison.  Zeros unless BCC_COMMIT_TIMING=1 was in the environment when
 * the library was loaded (measurement tools: tools/commit_bench.py). */
void bcc_commit_last_kernel_ms(double* ms3);

/* ---- tuple level with the CPubKey front end ---------------------------------------------------
 * verdict[i] = CPubKey(pub_i).Verify(msg_i, sig_i) (depend/bitcoin/src/pubkey.cpp:191-207) for n
 * tuples: pub_i = pub_blob[pub_off[i] .. pub_off[i+1]) (any length; the CPubKey length filter,
 * pubkey.h:58-94, applies), sig_i = sig_blob[sig_off[i] .. sig_off[i+1]) = DER without the
 * hashtype byte, parsed laxly (pubkey.cpp:28-168).  The blobs go to the GPU as they are and the
 * length filter and lax DER run there (K_der, csrc/der.hip), in pipelined rounds of 256k doubling
 * to 2M tuples; small rounds run on the host lane code.  Synchronous on `device`, or, for
 * device = -1, sharded in contiguous equal ranges over the bcc_set_devices() GPUs.  0, or -1 for
 * null arrays, offsets that are not non-decreasing (pub_off[i + 1] < pub_off[i] or
 * sig_off[i + 1] < sig_off[i] for any i: nothing is verified, so no verdict depends on how the call
 * is cut into rounds), or a device error. */
int bcc_pubkey_verify_batch(const uint8_t* pub_blob, const uint64_t* pub_off,
                            const uint8_t* msg32, const uint8_t* sig_blob,
                            const uint64_t* sig_off, uint8_t* verdict, size_t n, int device);

/* ---- engine configuration / statistics ---------------------------------------------------- */
/* Hash of the sources this library was built from (rust-bitcoinconsensus_amd/source_hash.py):
 * callers can check that the library they loaded matches the tree they test. */
const char* bcc_source_hash(void);

/* Device used by the bitcoinconsensus_* entry points of the calling process (default 0, or the
 * BCC_DEVICE environment variable). */
int bcc_set_device(int device);

/* Node sharding: spread every device round of bitcoinconsensus_verify_batch, and
 * bcc_pubkey_verify_batch(..., device = -1), over these GPUs (default: the single device above,
 * or BCC_DEVICES="0,1,2,..." in the environment; n = 0 restores the default).  A round is cut
 * into contiguous groups of whole transactions with about equal signature counts, one per GPU;
 * the groups run concurrently, each GPU from its own persistent host worker thread (its own HIP
 * stream, device arena and kernel scratch), and the verdicts are gathered on the host.  Results
 * never depend on the device set.  Returns 0, or -1 for a negative device id. */
int bcc_set_devices(const int* devices, int n);
/* Writes up to cap configured device ids to out; returns how many there are. */
int bcc_get_devices(int* out, int cap);

/* Lanes per signature-kernel launch (0 = default: 4M, or the BCC_CHUNK environment variable).
 * Bounds the per-caller device scratch (900 B per lane); results do not depend on it. */
int bcc_set_chunk_lanes(size_t lanes);

/* bitcoinconsensus_verify_batch pipelines a batch of at least two chunks: it is cut into chunks of
 * about `items` inputs (whole transactions), and each chunk's device round runs on a worker thread
 * while the host deserializes and interprets the next chunk.  Default 500000 (or the
 * BCC_PIPELINE_CHUNK environment variable); 0 disables it.  Results never depend on it. */
int bcc_set_pipeline_chunk(size_t items);
/* Items of a pipelined batch's last chunk (its device round is the one no host pass hides):
 * 0 (default, or BCC_PIPELINE_TAIL) keeps the remainder; results never depend on it. */
int bcc_set_pipeline_tail(size_t items);
/* Host shards per worker thread of a long bitcoinconsensus_verify_batch pass (default 1, or
 * BCC_LONG_SHARDS_PER_WORKER): with k > 1 the k x workers shards are dealt dynamically.  Results
 * never depend on it.  Returns 0, or -1 for k outside 1..64. */
int bcc_set_long_shards_per_worker(unsigned k);
/* bitcoinconsensus_verify_batch's first interpreter pass runs inside the parse pass, block by
 * block per host shard, while each item's transaction is still in cache (default 1, or
 * BCC_FUSED_PASS; 0: two passes).  Calls with early Q halves keep two passes.  Results never
 * depend on it.  Returns 0. */
int bcc_set_fused_pass(int on);
/* A device round's tuple rows, raw transactions and sighash blobs are written by the host pass into
 * page-locked memory and go to HBM from there, one copy per host shard and array; staging copies
 * only the records whose offsets it rebases (default 1, or BCC_DIRECT_UPLOAD; 0: every array is
 * copied into one pinned image first).  Results never depend on it.  Returns 0. */
int bcc_set_direct_upload(int on);
/* With the direct upload, each host shard of a pipelined bitcoinconsensus_verify_batch chunk sends
 * its tuple rows to the GPU as soon as the pass has finished it, and the chunk's device round
 * gathers them in HBM instead of uploading them (default 1, or BCC_PRE_UPLOAD).  Results never
 * depend on it.  Returns 0. */
int bcc_set_pre_upload(int on);

/* Legacy signature checks whose serial SHA-256 chain is longer than `blocks` 64-byte blocks (the
 * preimages of many-input transactions) are hashed on the host CPU instead of in one GPU lane each,
 * while the device round's message-independent kernels run (BCC_HOST_CHAIN_BLOCKS; default 160,
 * below the Q ladder's latency in GPU-lane blocks; 0: every legacy chain on the GPU).  A long
 * transaction template carries its SHA-256 midstates, so a check's chain counts only the blocks
 * from its own input's script on (host and GPU start from the midstate alike).  Single-GPU
 * rounds only, at most 2^19 blocks per interpreter pass.  BIP143 checks of a tx whose
 * per-tx chains (hashPrevouts / hashSequence / hashOutputs) exceed BCC_HOST_BIP143_BLOCKS (default
 * 32) blocks are hashed on the host (linear in the tx).  Results never depend on either. */
int bcc_set_host_chain_blocks(unsigned blocks);
/* The BIP143 threshold above (BCC_HOST_BIP143_BLOCKS; default 32; 0: every BIP143 chain on the GPU). */
int bcc_set_host_bip143_blocks(unsigned blocks);

/* Early Q halves (BCC_EARLY_Q; default 1): a verify_batch call that goes to one GPU as one chunk
 * (at most 2^18 inputs) pre-extracts the (key, signature) pairs of its standard spends after
 * deserialization and runs their key half and Q ladder on the GPU while the host interprets; the
 * interpreter's deferred checks with the same key and signature bytes reuse them.  0 disables it.
 * Results never depend on it. */
int bcc_set_early_q(int on);

/* Key-hash spends (P2WPKH, and P2PKH scriptPubKeys): on an input's first interpreter run the
 * HASH160(pubkey) == program comparison of OP_EQUALVERIFY is checked on the device beside the
 * signature (the row's verdict = signature valid AND hash equal); a false verdict re-runs the
 * input on the host with the comparison done there, so the error codes are the reference's.
 * on = 0: the host hashes every P2WPKH key before the run (BCC_DEVICE_KEY_HASH; default 1).
 * Results never depend on it. */
int bcc_set_device_key_hash(int on);

/* The remaining ECDSA-era hash types on the device-assembled paths: legacy NONE / SINGLE /
 * ANYONECANPAY checks (and their combinations) and BIP143 SIGHASH_SINGLE checks become device jobs
 * built from the raw transaction, which is uploaded once per round, instead of one host-serialized
 * preimage per check (O(inputs^2) bytes for a legacy transaction).  Default 0, or the
 * BCC_DEVICE_HASHTYPES environment variable: 0 keeps the host preimage path for them.  The
 * bcc_set_host_chain_blocks offload of long legacy chains applies either way.  Results never
 * depend on it.  Returns 0. */
int bcc_set_device_hashtypes(int on);

/* Host worker threads of a batch pass (verify_batch interpreter shards, tuple / Taproot front
 * ends, host-verified rounds).  0 restores the default: BCC_HOST_THREADS, else the CPUs of the
 * affinity mask, or the cgroup CPU quota when that is smaller, at most 64.  Results never
 * depend on it. */
int bcc_set_host_threads(unsigned n);
unsigned bcc_get_host_threads(void);
/* CPUs this process can keep busy: min(affinity mask, cgroup CPU quota). */
unsigned bcc_cpu_share(void);

/* bitcoinconsensus_verify_batch keeps its host-side state (items, parsed transactions, job
 * buffers) with the calling thread for reuse by its next call; batches above 4M items release it
 * on return.  bcc_taproot_verify_batch keeps its job buffers the same way, and every entry point
 * keeps a device batch (HBM arena, pinned staging image, streams, kernel scratch) per (thread,
 * GPU).  This releases the calling thread's state, and the state the library's own worker threads
 * keep (the per-GPU workers of a bcc_set_devices() list and the pipeline worker run rounds for
 * their callers), now.
 * Threads: with one device and no pipelining a call runs on the calling thread with that
 * thread's own device state, so concurrent callers share nothing.  With several devices
 * configured, or pipelining on, device rounds run on one shared worker thread per GPU: the results
 * are the same, but concurrent callers' rounds queue on those workers. */
void bcc_release_thread_state(void);

typedef struct bcc_batch_stats {
    size_t items, tuples, rounds, preimages, aux_messages, host_rejected;
    double host_seconds, gpu_seconds;
    /* breakdown: host deserialize + pre-checks, interpreter passes (preimage building
     * included), merging the per-thread rounds, host -> HBM staging (part of gpu_seconds) */
    double prepare_seconds, interpret_seconds, merge_seconds, stage_seconds;
    double total_seconds; /* the whole call, teardown included */
    size_t device_retries; /* device rounds that failed once and were re-run on a fresh batch */
    size_t devices;        /* GPUs a device round was spread over (max over the call's rounds) */
    size_t host_rounds;    /* rounds (or device groups) verified on the host CPU: small rounds
                            * (bcc_set_host_small_round) and device-failure fallbacks */
    size_t host_hashed;    /* deferred checks whose sighash the host computed (SHA chains longer
                            * than bcc_set_host_chain_blocks) */
    /* more of the host pass: shard / run lists, stitching verdicts into items, writing ret / err,
     * the host-hashed long chains */
    double shard_seconds, stitch_seconds, finish_seconds, host_jobs_seconds;
    /* the deserialization pass per worker, max over workers (summed over chunks): dispatch -> start
     * lag, tx parsing + pre-checks, the batched HASH160 of P2WPKH keys */
    double prepare_lag_seconds, prepare_parse_seconds, prepare_hash_seconds;
    /* key-hash conditions (HASH160(pubkey) == program) checked on the device beside their
     * signature (bcc_set_device_key_hash) */
    size_t device_key_hashes;
    /* interpreter passes per shard: the slowest shard and the mean (summed over passes): their
     * ratio is the passes' load imbalance */
    double interpret_shard_max_seconds, interpret_shard_mean_seconds;
    /* CPU time of the whole process (every thread) during the call, and during the caller's waits
     * for device rounds: under a CFS quota the first bounds back-to-back calls */
    double process_cpu_seconds, process_cpu_in_gpu_wait_seconds;
    /* early Q halves (bcc_set_early_q): pre-extracted rows whose key half and Q ladder ran on the
     * GPU during the host pass, the deferred rows mapped to them, and the extraction + launch time */
    size_t early_rows, early_mapped;
    double early_seconds;
    /* ... and the mapped rows whose legacy sighash came from the early set too (early sighashes:
     * long-template SIGHASH_ALL jobs hashed during the host pass, the round's copy skipped) */
    size_t early_msgs;
} bcc_batch_stats;
/* Statistics of the calling thread's last bitcoinconsensus_verify_batch / verify call. */
void bcc_last_batch_stats(bcc_batch_stats* out);

/* The deferred signature checks of a call by the way their sighash was computed: legacy
 * SIGHASH_ALL from the tx template, other legacy hash types from the raw tx
 * (bcc_set_device_hashtypes), BIP143 from the raw tx (SIGHASH_SINGLE counted apart; only with
 * bcc_set_device_hashtypes), a host-serialized preimage per check (legacy non-ALL types and BIP143
 * SIGHASH_SINGLE without bcc_set_device_hashtypes), legacy SIGHASH_SINGLE with n_in >= outputs
 * (no job: the message is uint256 ONE), and the checks the host hashed itself
 * (bcc_batch_stats.host_hashed). */
typedef struct bcc_sighash_kinds {
    size_t legacy_template, legacy_rawtx, bip143_rawtx, bip143_rawtx_single, host_preimage,
        single_bug, host_hashed;
} bcc_sighash_kinds;
/* The counts of the calling thread's last bitcoinconsensus_verify_batch / verify call, summed over
 * its rounds, or of its last bcc_debug_sighash call (include/bcc_bench.h), whichever was later. */
void bcc_last_sighash_kinds(bcc_sighash_kinds* out);

/* ---- host verification: the engine's own code on the CPU ------------------------------------
 * A device round (sighash jobs + ECDSA tuples) can be evaluated on the host with the engine's own
 * preimage builders, host SHA-256 and the kernels' lane code compiled for the CPU
 * (csrc/host/host_verify.cpp); the verdicts are the same.
 *
 * Device failure policy.  A failed device round is retried once on a fresh device batch when the
 * HIP error is transient (out of memory, not ready); a sticky error (launch failure, illegal
 * address, no device, ...) leaves the HIP context unusable, so it is not retried.  Then:
 *   BCC_DEVICE_FAILURE_HOST  (default; BCC_DEVICE_FAILURE=host) the round is verified on the host
 *                            CPU (logged on stderr, counted by bcc_host_fallback_rounds) and every
 *                            entry point returns its normal, exact result;
 *   BCC_DEVICE_FAILURE_ERROR (BCC_DEVICE_FAILURE=error) bitcoinconsensus_verify_batch returns -1
 *                            (unfinished items: BCC_ERR_DEVICE_FAILURE) and the single-item ABI
 *                            aborts, as there is no verdict (see bitcoinconsensus.h).
 * The Taproot entries follow the same rules with their own host evaluation
 * (csrc/host/taproot_host.cpp; see bcc_taproot_spend_batch). */
#define BCC_DEVICE_FAILURE_HOST 0
#define BCC_DEVICE_FAILURE_ERROR 1
int bcc_set_device_failure_policy(int policy);
/* Device rounds of at most `tuples` signature checks are verified on the host CPU with the
 * engine's own lane code instead of the GPU (default BCC_HOST_SMALL_ROUND_DEFAULT, or the
 * BCC_HOST_SMALL_ROUND environment variable; 0: every round on the GPU).  One lane of the GPU
 * ladder is a single wave issuing a few hundred thousand dependent instructions, so a lone
 * verify() costs ~1.6 ms as a GPU round and ~0.1 ms on the host.  The Taproot entries apply the
 * same threshold to their rounds (signature checks plus commitments); the figures measured for
 * them are in DESIGN.md 3.16. */
#define BCC_HOST_SMALL_ROUND_DEFAULT 16
int bcc_set_host_small_round(size_t tuples);
/* Device rounds (or per-GPU groups) verified on the host after a device failure, process-wide. */
size_t bcc_host_fallback_rounds(void);
/* mi_ecdsa_verify_tuples' contract on the host CPU (threads >= 1). */
int bcc_host_verify_tuples(const uint8_t* pub65, const uint8_t* msg32, const uint8_t* r32,
                           const uint8_t* s32, uint8_t* verdict, size_t n, unsigned threads);
/* mi_schnorr_verify_tuples' contract on the host CPU (threads >= 1): the kernels' BIP340 lane. */
int bcc_host_schnorr_verify_tuples(const uint8_t* sig64, const uint8_t* msg32,
                                   const uint8_t* xonly32, uint8_t* verdict, size_t n,
                                   unsigned threads);

/* Fault injection (tests): the next `rounds` device rounds of any thread fail as if the HIP
 * runtime had returned a transient error (hipErrorOutOfMemory), without touching the GPU (also:
 * BCC_FAULT_INJECT=rounds in the environment at load time); _code injects the given HIP error
 * (e.g. 719, hipErrorLaunchFailure: sticky, never retried).  Every device round of every entry
 * point counts, the Taproot ones included. */
void bcc_debug_fail_device_rounds(int rounds);
void bcc_debug_fail_device_rounds_code(int rounds, int hip_error);
/* Test hook: signature-kernel scratch requests above `lanes` lanes fail as out of memory (0: no
 * cap).  The kernels then run in the largest chunk that fits (halving from the request, at least
 * 64k lanes) instead of failing the round. */
void bcc_debug_scratch_cap_lanes(size_t lanes);

/* Test hook (coverage only): the shape a signature batch of n rows takes on a device with `cus`
 * compute units (cus <= 0: the current device's), computed by the helpers the launchers themselves
 * call, without launching or allocating anything.  A thread of K_inv / K_tfin walks the chain of
 * lanes t, t + T, t + 2 T, ... of its chunk and shares one inversion among them; *_threads is that
 * T.  BIP340 batches take the chunk stride and the K_tfin counts only (no K_inv, no K_keyq).
 * chunk_stride assumes the scratch fits on the device (else the launchers halve it).  Returns 0,
 * -1 for a null `out`, or a hipError_t value when the device cannot be asked. */
#define BCC_SHAPE_LATENCY 0    /* twist_keyq2_kernel: at most one wave per SIMD, two lanes a row */
#define BCC_SHAPE_ONE_LAUNCH 1 /* one K_keyq launch */
#define BCC_SHAPE_SPLIT 2      /* K_keyq as whole residency rounds [0, split_at) + a tail launch */
#define BCC_SHAPE_CHUNKED 3    /* n above the chunk stride: prep, ladder and K_tfin per chunk */
typedef struct bcc_launch_shape {
    size_t mode;              /* BCC_SHAPE_* (ECDSA) */
    size_t split_at;          /* A: first lane of the tail launch, 0 unless BCC_SHAPE_SPLIT */
    size_t chunk_stride;      /* C */
    size_t chunks;            /* ceil(n / C) */
    size_t inv_threads;       /* K_inv's T, over the whole batch */
    size_t fin_threads_first; /* K_tfin's T in the first chunk ... */
    size_t fin_threads_last;  /* ... and in the last one */
    size_t ladder_wg;         /* lanes per ladder workgroup */
    size_t inv_per_thread;    /* longest K_inv chain */
    size_t fin_per_thread;    /* longest K_tfin chain */
    size_t cus;
    size_t round_lanes;       /* R: lanes of one K_keyq residency round */
} bcc_launch_shape;
int bcc_debug_launch_shape(size_t n, int cus, bcc_launch_shape* out);
/* The same for the commitment kernels: tweak_fin_kernel's thread count T over a chunk of cnt rows
 * (its thread t walks lanes t, t + T, ... and shares one inversion among them). */
size_t bcc_debug_commit_fin_threads(size_t cnt);

#ifdef __cplusplus
}
#endif

#endif
