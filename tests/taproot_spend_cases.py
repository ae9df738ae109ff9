"""Builders and the loader for the whole-Taproot-input tests (bcc_taproot_spend_batch).

Two classes of cases, by what the reference can label:

  class R  spends that cannot reach a Schnorr verification.  Expected (ret, serror) is the
           reference's VerifyScript through Reference.capture_script, exactly as
           commit_cases.ref_spend asks it (the oracle builds its PrecomputedTransactionData without
           spent outputs and would assert on any Schnorr check, so the builders guarantee by
           construction that none is reached: no signature opcode meets a 32-byte key with a
           non-empty signature, and no key path signature is 64 or 65 bytes long).
  class S  spends with signatures.  No reference whole-spend verdict exists for them; the expected
           result is the rule of the entry point applied to the reference's per-check answers
           (Reference.taproot_check): the first non-empty signature, in execution order, whose
           check fails gives (0, its serror); else the template's own arithmetic.

Nothing here computes an expected value from the code under test; the curve and hash arithmetic of
commit_cases only constructs inputs."""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import commit_cases as C  # noqa: E402
import make_taproot_fixtures as G  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "taproot_spends.json.gz")
FLAGS = 0xE15 | 1 << 17
TAPSCRIPT = 1  # BCC_SIGVERSION_TAPSCRIPT
HASH_TYPES = [0, 1, 2, 3, 0x81, 0x82, 0x83]
# every error code the issue lists (script_error.h numbers)
LISTED_ERRORS = {2, 5, 7, 28, 29, 38, 40, 44, 45, 46, 47, 48, 49, 50}

OP_0, OP_1, OP_IF, OP_NOTIF, OP_ELSE, OP_ENDIF = b"\x00", b"\x51", b"\x63", b"\x64", b"\x67", b"\x68"
OP_DROP, OP_2DROP, OP_2DUP, OP_NOP, OP_NOT = b"\x75", b"\x6d", b"\x6e", b"\x61", b"\x91"
OP_NUMEQUAL, OP_CODESEP, OP_CHECKSIG, OP_CHECKSIGVERIFY = b"\x9c", b"\xab", b"\xac", b"\xad"
OP_CHECKMULTISIG, OP_CLTV, OP_CSV, OP_CHECKSIGADD = b"\xae", b"\xb1", b"\xb2", b"\xba"


# a well-encoded ECDSA signature (r = s = 1, SIGHASH_ALL) that verifies under no key
DER_SIG = bytes.fromhex("300602010102010101")


def push(d):
    """Minimal push of d (up to 0xffff bytes)."""
    if len(d) < 0x4c:
        return bytes([len(d)]) + d
    if len(d) <= 0xff:
        return b"\x4c" + bytes([len(d)]) + d
    return b"\x4d" + len(d).to_bytes(2, "little") + d


def num(n):
    """CScriptNum push of a small non-negative number."""
    if n == 0:
        return OP_0
    if n <= 16:
        return bytes([0x50 + n])
    b = bytearray()
    while n:
        b.append(n & 0xff)
        n >>= 8
    if b[-1] & 0x80:
        b.append(0)
    return push(bytes(b))


# ---- transactions ----------------------------------------------------------------------------
def place(rng, t, nin, program, witness, script_sig=b""):
    """Input nin of t spends OP_1 <program> with this witness."""
    t["vin"] = list(t["vin"])
    t["vin"][nin] = (t["vin"][nin][0], script_sig, t["vin"][nin][2])
    if t["wit"] is None:
        t["wit"] = [[] for _ in t["vin"]]
    t["wit"] = list(t["wit"])
    t["wit"][nin] = list(witness)
    if not any(t["wit"]):
        t["wit"] = None  # a witness flag without any witness does not deserialize
    t["spent"] = list(t["spent"])
    t["spent"][nin] = (t["spent"][nin][0], b"\x51\x20" + program)
    return t


def case_of(t, nin, cls, **kw):
    return dict(cls=cls, tx=G.tx_bytes(t), spent=G.ser_outs(t["spent"]), nin=nin, **kw)


def script_path(rng, script, stack, depth=None, leaf_version=0xC0, annex=None):
    """(program, witness, spend item) of a valid script-path spend of `script`."""
    it = C.make_spend(rng, rng.randrange(0, 4) if depth is None else depth, script, leaf_version)
    wit = list(stack) + [it["script"], it["control"]] + ([annex] if annex is not None else [])
    return it["program"], wit, it


def ref_whole(R, c):
    """Class R: the reference's VerifyScript for the case's input."""
    spk = _spent_script(c["spent"], c["nin"])
    ret, serr, _ = R.capture_script(spk, 0, c["tx"], c["nin"], FLAGS)
    return ret, serr


def _spent_script(spent, nin):
    """scriptPubKey nin of a serialized std::vector<CTxOut> (short compact sizes only)."""
    def rd(o):
        v = spent[o]
        if v < 253:
            return v, o + 1
        assert v == 253
        return int.from_bytes(spent[o + 1:o + 3], "little"), o + 3
    n, o = rd(0)
    for k in range(n):
        ln, o2 = rd(o + 8)
        if k == nin:
            return spent[o2:o2 + ln]
        o = o2 + ln
    raise IndexError(nin)


# ---- class R ---------------------------------------------------------------------------------
def weight_script(k, pad):
    """k signature checks of a 1-byte signature on a 33-byte key (an unknown key type: each
    passes unchecked and costs 50 of the budget), padded with `pad` NOPs; stack [sig, key]."""
    return (OP_2DUP + OP_CHECKSIG + OP_DROP) * k + OP_NOP * pad + OP_2DROP + OP_1


def class_r_specs(rng):
    """[(cls, dict(script, stack, ...))]: the fixed class R script-path cases."""
    k33, k31, k1, k32 = bytes([2]) * 33, bytes([3]) * 31, b"\x07", rng.randbytes(32)
    sig1 = b"\x01"
    S = []

    def add(cls, script, stack=(), **kw):
        S.append((cls, dict(script=script, stack=list(stack), **kw)))

    # OP_SUCCESSx: start, middle, end; after it nothing matters, before it everything must decode
    add("success_start", b"\x50")
    add("success_middle", OP_1 + b"\x62" + OP_0)
    add("success_end", OP_0 + OP_0 + b"\xfe")
    add("success_then_undecodable", b"\x7e" + b"\x4c")
    add("success_then_truncated_push", b"\xbb" + b"\x05\x01\x02")
    add("undecodable_then_success", b"\x4c\x50")
    add("truncated_push_then_success", b"\x03\x50\x50")
    add("success_overrides_limits", b"\x50", [bytes(521)] + [b""] * 1001)
    add("success_unexecuted_branch", OP_0 + OP_IF + b"\x89" + OP_ENDIF + OP_0)
    add("checksigadd_is_not_success", OP_0 + OP_0 + push(k33) + OP_CHECKSIGADD + OP_NOT)
    # CHECKMULTISIG
    add("checkmultisig", OP_0 + OP_0 + OP_0 + OP_CHECKMULTISIG)
    add("checkmultisigverify", OP_0 + OP_0 + OP_0 + b"\xaf" + OP_1)
    add("checkmultisig_unexecuted", OP_0 + OP_IF + OP_CHECKMULTISIG + OP_ENDIF + OP_1)
    # minimal IF
    for name, arg in (("01", b"\x01"), ("02", b"\x02"), ("0100", b"\x01\x00"), ("empty", b""),
                      ("00", b"\x00"), ("80", b"\x80")):
        add("minimalif_if_" + name, OP_IF + OP_1 + OP_ELSE + OP_1 + OP_ENDIF, [arg])
        add("minimalif_notif_" + name, OP_NOTIF + OP_1 + OP_ELSE + OP_1 + OP_ENDIF, [arg])
    add("minimalif_unexecuted", OP_0 + OP_IF + OP_IF + OP_ENDIF + OP_ENDIF + OP_1, [b"\x02"])
    # the validation weight budget (depth 0): the witness [sig(1), key(33), script(28), control(33)]
    # serializes to 1 + 2 + 34 + 29 + 34 = 100 bytes, so the budget is 150: three checks use it up
    # exactly, a fourth overdraws; an annex of 49 bytes (50 serialized) pays for the fourth
    add("weight_exact", weight_script(3, 17), [sig1, k33], depth=0)
    add("weight_one_too_many", weight_script(4, 14), [sig1, k33], depth=0)
    add("weight_annex_pays", weight_script(4, 14), [sig1, k33], depth=0, annex=b"\x50" + bytes(48))
    add("weight_annex_one_short", weight_script(4, 14), [sig1, k33], depth=0, annex=b"\x50" + bytes(47))
    add("weight_empty_sigs_are_free", weight_script(40, 0), [b"", k33], depth=0)
    # initial stack size, element size
    add("stack_1000", OP_2DROP * 500 + OP_1, [b""] * 1000)
    add("stack_1001", OP_2DROP * 500 + OP_DROP + OP_1, [b""] * 1001)
    add("stack_grows_past_1000", OP_1 + OP_2DROP * 500 + OP_DROP + OP_1, [b""] * 1000)
    add("element_520", OP_DROP + OP_1, [bytes([7]) * 520])
    add("element_521", OP_DROP + OP_1, [bytes([7]) * 521])
    add("push_521_in_script", b"\x4d\x09\x02" + bytes(521) + OP_DROP + OP_1)
    # no script size limit, no opcode limit
    add("script_10001_bytes_202_ops", OP_NOP * 10001 + OP_1)
    add("ops_202", OP_NOP * 202 + OP_1)
    add("script_big_pushes", (push(bytes(500)) + OP_DROP) * 25 + OP_1)
    # signature opcodes that reach no verification
    add("key_empty", OP_0 + OP_CHECKSIG, [sig1])
    add("key_empty_sig_empty", OP_0 + OP_CHECKSIG, [b""])
    add("key_empty_checksigadd", OP_0 + OP_0 + OP_CHECKSIGADD, [sig1])
    add("key_32_sig_empty", push(k32) + OP_CHECKSIG + OP_NOT, [b""])
    add("key_32_sig_empty_verify", push(k32) + OP_CHECKSIGVERIFY + OP_1, [b""])
    add("key_33_sig_any", push(k33) + OP_CHECKSIG, [rng.randbytes(64)])
    add("key_1_sig_any", push(k1) + OP_CHECKSIGVERIFY + OP_1, [sig1])
    add("key_31_sig_empty", push(k31) + OP_CHECKSIG, [b""])
    add("checksig_short_stack", OP_CHECKSIG, [sig1])
    for m in (1, 2, 3):  # two non-empty signatures on unknown key types, one empty on a 32-byte key
        add(f"checksigadd_count_{m}", push(k33) + OP_CHECKSIG + push(k32) + OP_CHECKSIGADD +
            push(k1) + OP_CHECKSIGADD + num(m) + OP_NUMEQUAL, [sig1, b"", rng.randbytes(64)])
    add("checksigadd_short_stack", push(k33) + OP_CHECKSIGADD, [sig1])
    add("checksigadd_big_num", push(k33) + OP_CHECKSIGADD, [sig1, bytes(5)])
    # clean stack and truth
    add("cleanstack_two", OP_1 + OP_1)
    add("cleanstack_empty", b"", [])
    add("empty_script_true", b"", [b"\x01"])
    add("eval_false", OP_0)
    add("eval_false_negative_zero", push(b"\x00\x80"))
    add("op_return", b"\x6a")
    add("unbalanced_if", OP_1 + OP_IF + OP_1)
    # lock times (the tx fields are set by the builder below)
    add("cltv_ok", num(100) + OP_CLTV + OP_DROP + OP_1, tx=dict(locktime=100, sequence=0))
    add("cltv_late", num(101) + OP_CLTV + OP_DROP + OP_1, tx=dict(locktime=100, sequence=0))
    add("cltv_final", num(100) + OP_CLTV + OP_DROP + OP_1, tx=dict(locktime=100, sequence=0xFFFFFFFF))
    add("cltv_negative", b"\x4f" + OP_CLTV + OP_DROP + OP_1, tx=dict(locktime=100, sequence=0))
    add("csv_ok", num(5) + OP_CSV + OP_DROP + OP_1, tx=dict(version=2, sequence=5))
    add("csv_early", num(6) + OP_CSV + OP_DROP + OP_1, tx=dict(version=2, sequence=5))
    add("csv_version_1", num(5) + OP_CSV + OP_DROP + OP_1, tx=dict(version=1, sequence=5))
    # annex: present, absent, and an element that only looks like one
    add("annex_present", OP_1, annex=b"\x50")
    add("annex_long", OP_DROP + OP_1, [b"\x50abc"], annex=b"\x50" + bytes(300))
    # leaf versions other than 0xc0: the script never runs
    for lv in (0xC2, 0x00, 0xFE, 0x50):
        add(f"leaf_version_{lv:02x}", b"\x6a" + rng.randbytes(5), [b"x"] * 3, leaf_version=lv)
    return S


def build_class_r(rng):
    """The fixed class R cases (no expected values: the caller asks the reference)."""
    out = []

    def tx_for(spec):
        t = G.make_tx(rng, nin=rng.randrange(1, 4), nout=rng.randrange(1, 3), long_ok=False)
        for k, v in spec.get("tx", {}).items():
            if k == "sequence":
                t["vin"] = [(p, s, v) for p, s, _ in t["vin"]]
            else:
                t[k] = v
        return t, rng.randrange(len(t["vin"]))

    for cls, spec in class_r_specs(rng):
        t, nin = tx_for(spec)
        prog, wit, _ = script_path(rng, spec["script"], spec["stack"], spec.get("depth"),
                                   spec.get("leaf_version", 0xC0), spec.get("annex"))
        out.append(case_of(place(rng, t, nin, prog, wit), nin, "r_" + cls))
    # commitment mutations and control sizes, with a script that would pass and one that would fail
    for script, tag in ((OP_1, "true"), (OP_0, "false")):
        base = C.make_spend(rng, 3, script + OP_NOP * 3, 0xC0)
        for what in C.applicable_mutations(base):
            it = C.mutate(rng, base, what)
            t, nin = tx_for({})
            out.append(case_of(place(rng, t, nin, it["program"], [it["script"], it["control"]]), nin,
                               f"r_mutate_{what}_{tag}"))
        for ln in (0, 1, 32, 34, 64, 33 + 32 * 3 - 1, 33 + 32 * 129):
            c = (base["control"] * 200)[:ln]
            t, nin = tx_for({})
            out.append(case_of(place(rng, t, nin, base["program"], [base["script"], c]), nin,
                               f"r_control_size_{ln}_{tag}"))
    it = C.mutate(rng, C.make_spend(rng, 2, b"\x6a", 0xC4), "node")
    t, nin = tx_for({})
    out.append(case_of(place(rng, t, nin, it["program"], [it["script"], it["control"]]), nin,
                       "r_unknown_leaf_version_mismatch"))
    # before the witness program: scriptSig, the program as a truth value, an empty witness
    good = script_path(rng, OP_1, [])
    for ss, tag in ((OP_1, "op1"), (OP_0, "op0"), (b"\x6a", "op_return"), (b"\x02\x01", "truncated"),
                    (OP_0 + OP_0 + OP_CHECKSIG, "checksig_empty_sig"),
                    # one ECDSA check of a well-encoded signature whose verdict is only pushed
                    (push(DER_SIG) + push(bytes([2]) * 33) + OP_CHECKSIG, "checksig_pushes_verdict"),
                    (push(DER_SIG) + push(bytes([2]) * 33) + OP_CHECKSIG + OP_DROP, "checksig_dropped"),
                    (push(DER_SIG[:-2] + b"\x01") + push(bytes([2]) * 33) + OP_CHECKSIG, "checksig_bad_der")):
        t, nin = tx_for({})
        out.append(case_of(place(rng, t, nin, good[0], good[1], script_sig=ss), nin, "r_scriptsig_" + tag))
    for prog, tag in ((bytes(32), "zero"), (bytes(31) + b"\x80", "negative_zero")):
        t, nin = tx_for({})
        out.append(case_of(place(rng, t, nin, prog, [OP_1, bytes([0xC0]) + bytes(32)]), nin,
                           "r_program_" + tag))
    for n_in in (1, 3):
        t = G.make_tx(rng, nin=n_in, nout=1, long_ok=False)
        nin = n_in - 1
        out.append(case_of(place(rng, t, nin, good[0], []), nin, f"r_witness_empty_{n_in}"))
    # key path without a possible verification: the size rule, hash_type 0 in 65 bytes
    for sig, tag in ((b"", "empty"), (rng.randbytes(63), "63"), (rng.randbytes(66), "66"),
                     (b"\x50" + bytes(9), "annex_alone"), (rng.randbytes(64) + b"\x00", "65_hashtype_0")):
        t, nin = tx_for({})
        out.append(case_of(place(rng, t, nin, rng.randbytes(32), [sig]), nin, "r_keypath_sig_" + tag))
    t, nin = tx_for({})
    out.append(case_of(place(rng, t, nin, rng.randbytes(32), [rng.randbytes(63), b"\x50\x01"]), nin,
                       "r_keypath_sig_63_annex"))
    return out


# ---- class S ---------------------------------------------------------------------------------
class Keys:
    """BIP340 key pairs and signatures from the reference's secp256k1."""

    def __init__(self, R, rng):
        self.R, self.rng = R, rng

    def new(self):
        sk = self.rng.randbytes(32)
        return sk, self.R.schnorr_sign(sk, bytes(32), bytes(32))[1]


def template(kind, keys, m=None, codesep=None):
    """(script, [(key index, codesep_pos)] in execution order, arithmetic) of a signature template.
    arithmetic(signed) -> (ret, serror) given which keys signed, when every signature is valid.
    codesep: None, "first" (before the first check), "between", "last" (after the last check)."""
    ops = []  # one entry per opcode
    checks = []
    pos = 0xFFFFFFFF

    def op(b):
        ops.append(b)

    def sep():
        nonlocal pos
        pos = len(ops)
        op(OP_CODESEP)

    if codesep == "first":
        sep()
    n = len(keys)
    for j, k in enumerate(keys):
        op(push(k))
        if kind == "verify_then_sig":
            op(OP_CHECKSIGVERIFY if j + 1 < n else OP_CHECKSIG)
        else:
            op(OP_CHECKSIG if j == 0 else OP_CHECKSIGADD)
        checks.append((j, pos))
        if codesep == "between" and j == 0:
            sep()
    if codesep == "last":
        sep()
    if kind == "multi":
        op(num(m))
        op(OP_NUMEQUAL)

    def arithmetic(signed):
        if kind == "verify_then_sig":
            for j in range(n - 1):
                if not signed[j]:
                    return 0, 13  # CHECKSIGVERIFY
            return (1, 0) if signed[n - 1] else (0, 2)
        if kind == "single":
            return (1, 0) if signed[0] else (0, 2)
        return (1, 0) if sum(signed) == m else (0, 2)

    return b"".join(ops), checks, arithmetic


def signed_spend(R, rng, t, nin, kind, nkeys, signers, hash_types, m=None, codesep=None,
                 annex=None, depth=None, tamper=None):
    """Places a signed script-path spend of a template on input nin of t (the tx's other fields
    are final: signatures commit to them).  signers[j]: key j signs.  tamper: None or
    (j, what) with what in sig_bit, sig_63, sig_66, hashtype_0, hashtype_bad (applied to signer j's
    signature after signing) or key_bit (key j in the script differs from the signer's).
    Returns dict(checks=[...], arith=(ret, serror)); the caller records the reference's answers."""
    K = Keys(R, rng)
    pairs = [K.new() for _ in range(nkeys)]
    if tamper and tamper[1] == "key_bit":  # the committed key differs from the signer's by one bit
        b = bytearray(pairs[tamper[0]][1])
        b[rng.randrange(32)] ^= 1 << rng.randrange(8)
        pairs[tamper[0]] = (pairs[tamper[0]][0], bytes(b))
    script, order, arithmetic = template(kind, [p[1] for p in pairs], m, codesep)
    prog, wit, it = script_path(rng, script, [], depth, 0xC0, annex)
    place(rng, t, nin, prog, wit)
    tx, spent = G.tx_bytes(t), G.ser_outs(t["spent"])
    sigs, checks = [b""] * nkeys, []
    for j, cpos in order:
        if not signers[j]:
            continue
        ht = hash_types[j]
        dummy = bytes(64) + (bytes([ht]) if ht else b"")
        _, _, h = R.taproot_check(tx, spent, nin, dummy, bytes(32), TAPSCRIPT, annex, it["leaf"], cpos)
        if h is None:  # SIGHASH_SINGLE without a matching output: nothing to sign
            sig = rng.randbytes(64) + bytes([ht])
        else:
            sig = R.schnorr_sign(pairs[j][0], h, rng.randbytes(32))[0] + (bytes([ht]) if ht else b"")
        if tamper and tamper[0] == j:
            what = tamper[1]
            if what == "sig_bit":
                b = bytearray(sig)
                b[rng.randrange(64)] ^= 1 << rng.randrange(8)
                sig = bytes(b)
            elif what == "sig_63":
                sig = sig[:63]
            elif what == "sig_66":
                sig = sig[:64] + b"\x01\x01"
            elif what == "hashtype_0":
                sig = sig[:64] + b"\x00"
            elif what == "hashtype_bad":
                sig = sig[:64] + b"\x04"
        sigs[j] = sig
        checks.append(dict(sig=sig, pk=pairs[j][1], codesep=cpos, leaf=it["leaf"], annex=annex))
    stack = list(reversed(sigs))  # the first key's signature on top
    wit = stack + [it["script"], it["control"]] + ([annex] if annex is not None else [])
    place(rng, t, nin, prog, wit)
    return dict(checks=checks, arith=arithmetic(signers))


def keypath_spend(R, rng, t, nin, ht, annex=None, tamper=None):
    sk, pk = Keys(R, rng).new()
    place(rng, t, nin, pk, [bytes(64)] + ([annex] if annex is not None else []))
    tx, spent = G.tx_bytes(t), G.ser_outs(t["spent"])
    dummy = bytes(64) + (bytes([ht]) if ht else b"")
    _, _, h = R.taproot_check(tx, spent, nin, dummy, bytes(32), 0, annex, bytes(32), 0xFFFFFFFF)
    if h is None:
        sig = rng.randbytes(64) + bytes([ht])
    else:
        sig = R.schnorr_sign(sk, h, rng.randbytes(32))[0] + (bytes([ht]) if ht else b"")
    if tamper == "sig_bit":
        b = bytearray(sig)
        b[rng.randrange(64)] ^= 1 << rng.randrange(8)
        sig = bytes(b)
    elif tamper == "key_bit":
        b = bytearray(pk)
        b[rng.randrange(32)] ^= 1 << rng.randrange(8)
        pk = bytes(b)
    elif tamper == "hashtype_bad":
        sig = sig[:64] + b"\x84"
    place(rng, t, nin, pk, [sig] + ([annex] if annex is not None else []))
    return dict(checks=[dict(sig=sig, pk=pk, codesep=0xFFFFFFFF, leaf=None, annex=annex)], arith=(1, 0))


def s_tx(rng, ht_max_single=False, nin=None):
    """A tx for signed spends: enough outputs for SIGHASH_SINGLE unless asked otherwise."""
    t = G.make_tx(rng, nin=nin if nin is not None else rng.randrange(1, 4), nout=rng.randrange(1, 4),
                  long_ok=False)
    if not ht_max_single and len(t["vout"]) < len(t["vin"]):
        t["vout"] = t["vout"] + [(1000, b"\x51")] * (len(t["vin"]) - len(t["vout"]))
    t["vin"] = [(p, b"", s) for p, _, s in t["vin"]]
    return t


def label_s(R, c):
    """Records the reference's per-check answers in a class S case and returns its expected
    (ret, serror): the first failing check's, else the template's arithmetic."""
    exp = tuple(c["arith"])
    first = None
    for k in c["checks"]:
        sv = 0 if k["leaf"] is None else TAPSCRIPT
        ret, serr, _ = R.taproot_check(c["tx"], c["spent"], c["nin"], k["sig"], k["pk"], sv,
                                       k["annex"], k["leaf"] or bytes(32), k["codesep"])
        k["ref"] = (ret, serr)
        if ret != 1 and first is None:
            first = (0, serr)
    return first if first is not None else exp


def expected_s(c):
    """The same rule from the recorded answers (golden cases)."""
    for k in c["checks"]:
        if k["ref"][0] != 1:
            return 0, k["ref"][1]
    return tuple(c["arith"])


def build_class_s(R, rng):
    """The fixed class S cases, labelled by the reference's per-check answers."""
    out = []

    def emit(t, nin, cls, info):
        c = case_of(t, nin, "s_" + cls, checks=info["checks"], arith=info["arith"])
        # a tampered check stops the script: checks after it were never reached
        c["expected"] = label_s(R, c)
        out.append(c)
        return c

    for ht in HASH_TYPES:
        for annex in (None, b"\x50" + rng.randbytes(rng.randrange(0, 70))):
            t = s_tx(rng)
            nin = rng.randrange(len(t["vin"]))
            emit(t, nin, f"keypath_{ht:02x}", keypath_spend(R, rng, t, nin, ht, annex))
            t = s_tx(rng)
            nin = rng.randrange(len(t["vin"]))
            emit(t, nin, f"checksig_{ht:02x}",
                 signed_spend(R, rng, t, nin, "single", 1, [True], [ht], annex=annex))
    for tamper in ("sig_bit", "key_bit", "hashtype_bad"):
        t = s_tx(rng)
        emit(t, 0, "keypath_" + tamper, keypath_spend(R, rng, t, 0, 1, tamper=tamper))
    for what in ("sig_bit", "sig_63", "sig_66", "hashtype_0", "hashtype_bad"):
        t = s_tx(rng)
        emit(t, 0, "checksig_" + what,
             signed_spend(R, rng, t, 0, "single", 1, [True], [1], tamper=(0, what)))
    for kind, nk, j in (("single", 1, 0), ("multi", 3, 1), ("verify_then_sig", 2, 1)):
        t = s_tx(rng)
        emit(t, 0, f"{'checksig' if kind == 'single' else kind}_key_bit",
             signed_spend(R, rng, t, 0, kind, nk, [True] * nk, [0] * nk, m=nk, tamper=(j, "key_bit")))
    # SIGHASH_SINGLE without a matching output
    for kind in ("keypath", "checksig"):
        t = s_tx(rng, ht_max_single=True, nin=3)
        t["vout"] = t["vout"][:1]
        if kind == "keypath":
            emit(t, 2, "keypath_single_no_output", keypath_spend(R, rng, t, 2, 3))
        else:
            emit(t, 2, "checksig_single_no_output",
                 signed_spend(R, rng, t, 2, "single", 1, [True], [0x83]))
    # a signed field of the tx changes after signing
    t = s_tx(rng)
    info = signed_spend(R, rng, t, 0, "single", 1, [True], [0])
    t["locktime"] ^= 1
    emit(t, 0, "checksig_tx_bit", info)
    t = s_tx(rng)
    info = keypath_spend(R, rng, t, 0, 0)
    t["locktime"] ^= 1
    emit(t, 0, "keypath_tx_bit", info)
    # CHECKSIGVERIFY then CHECKSIG
    for signers in ([True, True], [False, True], [True, False]):
        for cs_ in (None, "first", "between", "last"):
            t = s_tx(rng)
            nin = rng.randrange(len(t["vin"]))
            emit(t, nin, f"verify_then_sig_{int(signers[0])}{int(signers[1])}_{cs_}",
                 signed_spend(R, rng, t, nin, "verify_then_sig", 2, signers,
                              [rng.choice(HASH_TYPES[:3]) for _ in range(2)], codesep=cs_))
    t = s_tx(rng)
    emit(t, 0, "verify_then_sig_first_bad",
         signed_spend(R, rng, t, 0, "verify_then_sig", 2, [True, True], [0, 0], tamper=(0, "sig_bit")))
    t = s_tx(rng)
    emit(t, 0, "verify_then_sig_second_size",
         signed_spend(R, rng, t, 0, "verify_then_sig", 2, [True, True], [0, 0], tamper=(1, "sig_63")))
    # m of n
    for n, m, signers in ((3, 2, [1, 0, 1]), (3, 2, [1, 1, 1]), (3, 2, [0, 0, 1]), (5, 3, [0, 1, 1, 0, 1]),
                          (2, 2, [1, 1]), (4, 1, [0, 0, 0, 0])):
        for cs_ in (None, "first", "between", "last"):
            t = s_tx(rng)
            nin = rng.randrange(len(t["vin"]))
            emit(t, nin, f"multi_{m}of{n}_{''.join(map(str, signers))}_{cs_}",
                 signed_spend(R, rng, t, nin, "multi", n, [bool(s) for s in signers],
                              [rng.choice(HASH_TYPES) for _ in range(n)], m=m, codesep=cs_,
                              annex=rng.choice([None, b"\x50\x00"])))
    for j, what in ((0, "sig_bit"), (2, "sig_bit"), (1, "sig_66"), (2, "hashtype_0")):
        t = s_tx(rng)
        emit(t, 0, f"multi_3of3_tamper_{j}_{what}",
             signed_spend(R, rng, t, 0, "multi", 3, [True] * 3, [0, 1, 0x81], m=3, tamper=(j, what)))
    return out


def script_bit_cases(R, rng):
    """Signed spends whose script loses one bit after signing: the commitment no longer holds, no
    check is reached, so these are class R (the reference's VerifyScript labels them)."""
    out = []
    for kind, nk in (("single", 1), ("multi", 3)):
        t = s_tx(rng)
        signed_spend(R, rng, t, 0, kind, nk, [True] * nk, [0] * nk, m=nk, depth=2)
        wit = list(t["wit"][0])
        b = bytearray(wit[-2])
        b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
        wit[-2] = bytes(b)
        t["wit"][0] = wit
        out.append(case_of(t, 0, f"r_signed_{kind}_script_bit"))
    return out


def multi_input_cases(R, rng, n_in=4):
    """Adjacent items of ONE tx, one spend per input (they share the tx and spent bytes objects):
    key path and script templates mixed.  The tx is final before anything signs."""
    t = s_tx(rng, nin=n_in)
    infos = []
    # every input's program and witness shape must be placed before signing any (sha_scriptpubkeys
    # covers all spent outputs), so sign in two passes: place dummies, then sign each
    plans = []
    for nin in range(n_in):
        plans.append(rng.choice(["keypath", "single", "multi"]))
    # pass 1: programs (fresh keys per input are made inside the builders, so run them twice with
    # the same per-input generator state)
    import random as _random
    seeds = [rng.getrandbits(64) for _ in range(n_in)]
    for _ in range(2):
        infos = []
        for nin, plan in enumerate(plans):
            r2 = _random.Random(seeds[nin])
            if plan == "keypath":
                infos.append(keypath_spend(R, r2, t, nin, 0))
            elif plan == "single":
                infos.append(signed_spend(R, r2, t, nin, "single", 1, [True], [1]))
            else:
                infos.append(signed_spend(R, r2, t, nin, "multi", 3, [True, False, True], [0, 0, 2], m=2))
    tx, spent = G.tx_bytes(t), G.ser_outs(t["spent"])
    out = []
    for nin, info in enumerate(infos):
        c = dict(cls=f"s_multi_input_{plans[nin]}", tx=tx, spent=spent, nin=nin, checks=info["checks"],
                 arith=info["arith"])
        c["expected"] = label_s(R, c)
        out.append(c)
    return out


# ---- random spends of both classes (live reference) ------------------------------------------
def random_cases(R, rng, n):
    """n fresh spends, about half of them valid, every listed error code reachable; expected from
    the live reference (class R: VerifyScript; class S: the per-check rule)."""
    out = []
    r_pool = None
    while len(out) < n:
        k = rng.random()
        if k < 0.30:  # class S, mostly valid
            t = s_tx(rng)
            nin = rng.randrange(len(t["vin"]))
            ht = rng.choice(HASH_TYPES)
            tam = rng.choice([None, None, None, "sig_bit"])
            if rng.random() < 0.4:
                info = keypath_spend(R, rng, t, nin, ht, rng.choice([None, b"\x50\x01"]), tam)
            elif rng.random() < 0.5:
                info = signed_spend(R, rng, t, nin, "single", 1, [True], [ht],
                                    tamper=(0, rng.choice(["sig_bit", "sig_63", "hashtype_0"])) if tam else None)
            else:
                nk = rng.randrange(2, 5)
                signers = [rng.random() < 0.7 for _ in range(nk)]
                m = sum(signers) if rng.random() < 0.8 else nk + 1
                info = signed_spend(R, rng, t, nin, "multi", nk, signers,
                                    [rng.choice(HASH_TYPES[:3]) for _ in range(nk)], m=m,
                                    codesep=rng.choice([None, "first", "between", "last"]),
                                    tamper=(rng.randrange(nk), "sig_bit") if tam else None)
            c = case_of(t, nin, "s_random", checks=info["checks"], arith=info["arith"])
            c["expected"] = label_s(R, c)
            out.append(c)
        else:  # class R: a fresh instance of the fixed shapes (new keys, paths, txs)
            if not r_pool:
                r_pool = build_class_r(rng)
                rng.shuffle(r_pool)
            c = r_pool.pop()
            c["expected"] = ref_whole(R, c)
            out.append(c)
    return out


# ---- golden file -----------------------------------------------------------------------------
def _hex(b):
    return None if b is None else b.hex()


def _unhex(s):
    return None if s is None else bytes.fromhex(s)


def dump_golden(cases, path=GOLDEN):
    blobs, index = [], {}

    def ref(b):
        h = b.hex()
        if h not in index:
            index[h] = len(blobs)
            blobs.append(h)
        return index[h]

    rows = []
    for c in cases:
        row = dict(cls=c["cls"], tx=ref(c["tx"]), spent=ref(c["spent"]), nin=c["nin"],
                   ret=c["expected"][0], serror=c["expected"][1])
        if "checks" in c:
            row["arith"] = list(c["arith"])
            row["checks"] = [dict(sig=k["sig"].hex(), pk=k["pk"].hex(), codesep=k["codesep"],
                                  leaf=_hex(k["leaf"]), annex=_hex(k["annex"]), ref=list(k["ref"]))
                             for k in c["checks"]]
        rows.append(row)
    with gzip.open(path, "wt") as f:
        json.dump(dict(source="oracle/_ref: ref_capture_script (VerifyScript, class r_*) and "
                              "ref_taproot_check (CheckSchnorrSignature, the checks of class s_*)",
                       flags=FLAGS, blobs=blobs, cases=rows), f, separators=(",", ":"))


_loaded = None


def load_golden():
    """The golden cases: dicts cls, tx, spent, nin, expected=(ret, serror), and for class S the
    checks (sig, pk, codesep, leaf, annex, ref) and arith.  Adjacent cases of one tx share the tx
    and spent bytes objects."""
    global _loaded
    if _loaded is None:
        with gzip.open(GOLDEN, "rt") as f:
            d = json.load(f)
        blobs = [bytes.fromhex(b) for b in d["blobs"]]
        out = []
        for r in d["cases"]:
            c = dict(cls=r["cls"], tx=blobs[r["tx"]], spent=blobs[r["spent"]], nin=r["nin"],
                     expected=(r["ret"], r["serror"]))
            if "checks" in r:
                c["arith"] = tuple(r["arith"])
                c["checks"] = [dict(sig=bytes.fromhex(k["sig"]), pk=bytes.fromhex(k["pk"]),
                                    codesep=k["codesep"], leaf=_unhex(k["leaf"]),
                                    annex=_unhex(k["annex"]), ref=tuple(k["ref"]))
                               for k in r["checks"]]
                assert c["expected"] == expected_s(c), c["cls"]
            out.append(c)
        _loaded = out
    return _loaded


def items_of(cases):
    return [dict(tx=c["tx"], spent=c["spent"], nin=c["nin"]) for c in cases]
