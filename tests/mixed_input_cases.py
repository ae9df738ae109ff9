"""Cases for bcc_verify_inputs_batch (include/bcc_amd.h): any input against the outputs its
transaction spends, v1 and older kinds in one call.

Every case is a dict with tx, spent (the serialized std::vector<CTxOut> the whole tx spends), nin,
flags, expected = (ret, err) of the entry point's contract, v1 (True where the contract routes the
item to the Taproot side: TAPROOT set, rules 1-3 passed, spent[nin] exactly OP_1 0x20 <32 bytes>)
and cls.  Classes:

  lifted_cases()    the 4,207 rows of script_cases.json.gz lifted to (tx, spent, nin): the row's
                    (amount, spk) at nin, arbitrary outputs elsewhere; expected = the row's recorded
                    reference answer; the 0xE15 rows again with | 1 << 17 (none spends a native v1
                    program, so TAPROOT changes nothing for them).
  taproot_cases()   the 216 cases of taproot_spends.json.gz: with TAPROOT their recorded verdict and
                    err 0; with 0xE15 what the reference's verify_script_with_amount answers (v1
                    passes unchecked), recorded in mixed_inputs.json.gz.
  mixed_cases()     the mixed transactions of mixed_inputs.json.gz (golden/make_mixed_inputs_
                    fixtures.py): 2-4 inputs of seven kinds, about 1 in 4 tampered, every input
                    relabelled after the tamper.  Non-v1 inputs carry the reference's
                    verify_script_with_amount answer at 0xE15, v1 inputs taproot_spend_cases.label_s's
                    rule over the reference's per-check answers.
  contract_cases()  rules 1-3 and their order, built here from a golden transaction; the expected
                    values are the contract's, and the fixture generator asserts that the reference
                    names the same transaction error for each.

build_mixed_tx / label_mixed construct and label fresh mixed transactions with a live reference
(the generator, the random GPU test and tools/inputs_bench.py).  Nothing here computes an expected
value from the code under test."""
import gzip
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import taproot_spend_cases as S  # noqa: E402
from script_asm import hash160  # noqa: E402

G = S.G
GOLDEN = os.path.join(HERE, "golden", "mixed_inputs.json.gz")
ALL = 0xE15
TAPROOT = 1 << 17
ERR_TX_INDEX, ERR_TX_SIZE_MISMATCH, ERR_TX_DESERIALIZE, ERR_INVALID_FLAGS = 1, 2, 3, 5
ERR_SPENT_OUTPUTS_MISMATCH = 7

ECDSA_KINDS = ["p2pkh", "p2wpkh", "p2sh_p2wpkh", "p2wsh_2of3", "p2sh_2of3"]
V1_KINDS = ["tr_key", "tr_script"]
KINDS = ECDSA_KINDS + V1_KINDS
TAMPERS = ["sig_bit", "key_bit", "amount", "other_spk"]


def is_v1(spk):
    return len(spk) == 34 and spk[0] == 0x51 and spk[1] == 0x20


def case(tx, spent, nin, flags, expected, cls, v1=False):
    return dict(tx=tx, spent=spent, nin=nin, flags=flags, expected=tuple(expected), cls=cls, v1=v1)


# ---- lifted script cases -----------------------------------------------------------------------
def input_count(tx):
    """vin.size() as UnserializeTransaction reads it (primitives/transaction.h:188-224), or None
    where the bytes end first.  Only shapes the lifted blob: a wrong count would show as a failure
    against the row's recorded reference answer."""
    def cs(o):
        if o >= len(tx):
            return None
        v = tx[o]
        if v < 253:
            return v
        w = {253: 2, 254: 4, 255: 8}[v]
        return int.from_bytes(tx[o + 1:o + 1 + w], "little") if o + 1 + w <= len(tx) else None
    n = cs(4)
    if n == 0 and len(tx) > 5 and tx[5] != 0:  # marker 0x00, flag: the real vin follows
        n = cs(6)
    return n


def lift(spk, amount, tx, nin, filler=b"\x6a"):
    """The spent-outputs blob of a script_cases row: (amount, spk) at nin, (1000 + k, OP_RETURN)
    elsewhere, one per input; any blob where the tx does not parse or nin is out of range."""
    n = input_count(tx)
    if n is None or n > 10000:
        return G.ser_outs([(amount, spk)])
    outs = [(1000 + k, filler) for k in range(n)]
    if nin < n:
        outs[nin] = (amount, spk)
    return G.ser_outs(outs)


_lifted = None


def lifted_cases():
    global _lifted
    if _lifted is None:
        with gzip.open(os.path.join(HERE, "golden", "script_cases.json.gz"), "rt") as f:
            rows = json.load(f)
        out, txs = [], {}
        for r in rows:
            spk = bytes.fromhex(r["spk"])
            tx = txs.setdefault(r["tx"], bytes.fromhex(r["tx"]))
            assert not is_v1(spk), r["src"]  # no row is left out: none spends a native v1 program
            spent = lift(spk, r["amount"], tx, r["nin"])
            out.append(case(tx, spent, r["nin"], r["flags"], (r["ret"], r["err"]), "lifted:" + r["src"]))
            if r["flags"] == ALL:
                out.append(case(tx, spent, r["nin"], ALL | TAPROOT, (r["ret"], r["err"]),
                                "lifted_tr:" + r["src"]))
        _lifted = out
    return _lifted


# ---- the fixture -------------------------------------------------------------------------------
_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with gzip.open(GOLDEN, "rt") as f:
            _fixture = json.load(f)
    return _fixture


def taproot_cases():
    """The Taproot goldens under both flag sets."""
    gold = S.load_golden()
    plain = fixture()["taproot_spends_at_0xE15"]
    assert len(plain) == len(gold)
    out = []
    for c, p in zip(gold, plain):
        assert c["expected"][0] in (0, 1)
        out.append(case(c["tx"], c["spent"], c["nin"], ALL | TAPROOT, (c["expected"][0], 0),
                        "tr:" + c["cls"], v1=True))
        out.append(case(c["tx"], c["spent"], c["nin"], ALL, tuple(p), "tr_plain:" + c["cls"]))
    return out


def mixed_txs():
    """The fixture's transactions: dicts tx, spent, inputs = [dict(kind, tamper, ret)]."""
    return [dict(tx=bytes.fromhex(t["tx"]), spent=bytes.fromhex(t["spent"]), inputs=t["inputs"],
                 tamper=t["tamper"]) for t in fixture()["mixed"]]


def cases_of_tx(t, cls="mixed"):
    """One case per input; the inputs of one tx share the tx and spent bytes objects."""
    return [case(t["tx"], t["spent"], k, ALL | TAPROOT, (i["ret"], 0), f"{cls}:{i['kind']}",
                 v1=i["kind"] in V1_KINDS) for k, i in enumerate(t["inputs"])]


def mixed_cases():
    return [c for t in mixed_txs() for c in cases_of_tx(t)]


# ---- contract cases ----------------------------------------------------------------------------
def tx_variants(tx, n_in):
    """(tag, tx bytes, nin, E_tx) of each transaction error, nin 0 otherwise."""
    return [("deserialize", tx[:len(tx) // 2], 0, ERR_TX_DESERIALIZE),
            ("empty_tx", b"", 0, ERR_TX_DESERIALIZE),
            ("index", tx, n_in, ERR_TX_INDEX),
            ("index_far", tx, 0xFFFFFFFF, ERR_TX_INDEX),
            ("size", tx + b"\x00", 0, ERR_TX_SIZE_MISMATCH)]


def contract_bases():
    """(tag, tx, spent, input count) of a v1 and a non-v1 base: mixed transactions of the fixture
    whose input 0 is of that kind and valid."""
    out = []
    for tag, kinds in (("v1", V1_KINDS), ("ecdsa", ECDSA_KINDS)):
        t = next(t for t in mixed_txs() if t["inputs"][0]["kind"] in kinds and t["inputs"][0]["ret"] == 1)
        out.append((tag, t["tx"], t["spent"], len(t["inputs"])))
    return out


def contract_cases():
    out = []
    f = ALL | TAPROOT
    zero_in = G.ser_tx(1, [], [], 0)                       # 0 inputs, 0 outputs: parses, no index
    marker = bytes.fromhex("01000000" "0001" "00" "00" "00000000")  # witness flag, no inputs
    for tag, tx, spent, n in contract_bases():
        v1 = tag == "v1"
        out.append(case(tx, spent, 0, f, (1, 0), f"{tag}:base", v1=v1))
        # rule 2: each E_tx
        for name, tx2, nin, e in tx_variants(tx, n):
            out.append(case(tx2, spent, nin, f, (0, e), f"{tag}:etx_{name}"))
        # rule 3: truncated, one trailing byte, count - 1, count + 1, empty
        outs = spent[1:]
        one = outs[:8 + 1 + outs[8]]
        bad = [("truncated", spent[:-1]), ("trailing", spent + b"\x00"),
               ("count_less", bytes([n - 1]) + outs if n > 1 else b"\x00"),
               ("count_more", bytes([n + 1]) + outs + one),
               ("count_less_parses", bytes([n - 1]) + outs[:len(outs) - _last_len(outs, n)]),
               ("count_more_short", bytes([n + 1]) + outs), ("empty", b""), ("zero", b"\x00")]
        for name, sp in bad:
            out.append(case(tx, sp, 0, f, (0, ERR_SPENT_OUTPUTS_MISMATCH), f"{tag}:spent_{name}"))
        # precedence: E_tx before the mismatch (nin >= count is TX_INDEX, whatever the blob)
        for name, tx2, nin, e in tx_variants(tx, n):
            out.append(case(tx2, spent + b"\x00", nin, f, (0, e), f"{tag}:etx_{name}_over_mismatch"))
        out.append(case(tx, b"", n, f, (0, ERR_TX_INDEX), f"{tag}:index_over_empty"))
        # rule 1 before everything
        for name, fl in (("taproot_without_cltv", TAPROOT | (ALL & ~(1 << 9))), ("taproot_alone", TAPROOT),
                         ("unknown_bit", ALL | 1 << 1), ("taproot_unknown_bit", ALL | TAPROOT | 1 << 20)):
            out.append(case(tx, spent, 0, fl, (0, ERR_INVALID_FLAGS), f"{tag}:flags_{name}"))
            out.append(case(tx[:9], b"", 9, fl, (0, ERR_INVALID_FLAGS), f"{tag}:flags_{name}_bad_item"))
    for name, tx in (("zero_inputs", zero_in), ("marker_no_inputs", marker)):
        for sp in (b"\x00", b"", G.ser_outs([(1, b"\x51\x20" + bytes(32))])):
            out.append(case(tx, sp, 0, f, (0, None), f"tx:{name}:{len(sp)}"))
    # a v1 input whose scriptSig holds two ECDSA checks of non-empty signatures:
    # bcc_taproot_spend_batch answers -1; invalid under every verdict, so ret 0 / err 0 here
    import random
    rng = random.Random(3)
    prog, wit, _ = S.script_path(rng, S.OP_1, [])
    key = S.push(bytes([2]) * 33)
    for name, ss in (("checksigverify", S.push(S.DER_SIG) + key + S.OP_CHECKSIGVERIFY),
                     ("two_checksigs", (S.push(S.DER_SIG) + key + S.OP_CHECKSIG) * 2)):
        t = G.make_tx(rng, nin=1, nout=1, long_ok=False)
        S.place(rng, t, 0, prog, wit, script_sig=ss)
        out.append(case(G.tx_bytes(t), G.ser_outs(t["spent"]), 0, f, (0, 0), "v1:scriptsig_" + name,
                        v1=True))
    return out


def _last_len(outs, n):
    """Serialized size of the last of n short outputs."""
    o = 0
    for _ in range(n):
        ln = 9 + outs[o + 8]
        o += ln
    return ln


def resolve_tx_cases(cases, etx):
    """The E_tx of the zero-input and the witness-marker transaction is the reference's recorded
    answer (fixture key contract_etx, by name): fills the cases built with err None."""
    return [dict(c, expected=(0, etx[c["cls"].split(":")[1]])) if c["expected"][1] is None else c
            for c in cases]


def all_contract_cases():
    return resolve_tx_cases(contract_cases(), fixture()["contract_etx"])


# ---- building mixed transactions (live reference) ---------------------------------------------
def _wit(t):
    if t["wit"] is None:
        t["wit"] = [[] for _ in t["vin"]]
    t["wit"] = [list(w) for w in t["wit"]]
    return t["wit"]


def _bytes(t):
    t = dict(t)
    if t["wit"] is not None and not any(t["wit"]):
        t["wit"] = None
    return G.tx_bytes(t)


def _flip(b, rng, lo, hi):
    b = bytearray(b)
    b[rng.randrange(lo, hi)] ^= 1 << rng.randrange(8)
    return bytes(b)


def ecdsa_input(R, O, rng, t, nin, kind, tamper=None):
    """Places a signed spend of `kind` on input nin (SIGHASH_ALL, signed by the reference over the
    oracle's sighash of the tx as it stands).  tamper: sig_bit or key_bit, applied after signing."""
    sks = [rng.randbytes(32) for _ in range(3)]
    pubs = [R.pubkey_create(sk, compressed=(kind != "p2pkh" or rng.random() < 0.5)) for sk in sks]
    amount = t["spent"][nin][0]
    multi = b"\x52" + b"".join(S.push(p) for p in pubs) + b"\x53\xae"
    h = hash160(pubs[0])
    pkh = b"\x76\xa9\x14" + h + b"\x88\xac"
    script_sig = b""
    if kind == "p2pkh":
        spk, code, sv = pkh, pkh, 0
    elif kind == "p2wpkh":
        spk, code, sv = b"\x00\x14" + h, pkh, 1
    elif kind == "p2sh_p2wpkh":
        redeem = b"\x00\x14" + h
        spk, code, sv, script_sig = b"\xa9\x14" + hash160(redeem) + b"\x87", pkh, 1, S.push(redeem)
    elif kind == "p2wsh_2of3":
        spk, code, sv = b"\x00\x20" + hashlib.sha256(multi).digest(), multi, 1
    elif kind == "p2sh_2of3":
        spk, code, sv = b"\xa9\x14" + hash160(multi) + b"\x87", multi, 0
    else:
        raise ValueError(kind)
    t["spent"] = list(t["spent"])
    t["spent"][nin] = (amount, spk)
    t["vin"] = list(t["vin"])
    prev, _, seq = t["vin"][nin]
    t["vin"][nin] = (prev, script_sig, seq)
    wit = _wit(t)
    wit[nin] = []
    m = O.sighash(_bytes(t), nin, code, 1, amount, sv)
    signers = [0] if kind in ("p2pkh", "p2wpkh", "p2sh_p2wpkh") else sorted(rng.sample(range(3), 2))
    sigs = [R.sign(sks[j], m) + b"\x01" for j in signers]
    if tamper == "sig_bit":
        sigs[-1] = _flip(sigs[-1], rng, len(sigs[-1]) - 21, len(sigs[-1]) - 1)
    if tamper == "key_bit":
        pubs[0] = _flip(pubs[0], rng, 1, 33)
        multi = b"\x52" + b"".join(S.push(p) for p in pubs) + b"\x53\xae"
    if kind == "p2pkh":
        script_sig = S.push(sigs[0]) + S.push(pubs[0])
    elif kind in ("p2wpkh", "p2sh_p2wpkh"):
        wit[nin] = [sigs[0], pubs[0]]
    elif kind == "p2wsh_2of3":
        wit[nin] = [b""] + sigs + [multi]
    else:
        script_sig = b"\x00" + b"".join(S.push(s) for s in sigs) + S.push(multi)
    t["vin"][nin] = (prev, script_sig, seq)
    return dict(kind=kind)


def v1_input(R, rng, t, nin, kind, ht, tamper=None):
    """A Taproot key-path or script-path spend (taproot_spend_cases' builders) on input nin."""
    if kind == "tr_key":
        info = S.keypath_spend(R, rng, t, nin, ht, tamper=tamper)
    else:
        tpl, nk = rng.choice([("single", 1), ("multi", 2), ("multi", 3), ("verify_then_sig", 2)])
        j = rng.randrange(nk)
        info = S.signed_spend(R, rng, t, nin, tpl, nk, [True] * nk,
                              [ht if k == 0 else rng.choice(S.HASH_TYPES[:3]) for k in range(nk)], m=nk,
                              codesep=rng.choice([None, None, "first", "between"]),
                              tamper=(j, tamper) if tamper else None)
    return dict(kind=kind, checks=info["checks"], arith=info["arith"])


def build_mixed_tx(R, O, rng, kinds, tampers=None, hash_types=None):
    """A transaction with one input per entry of `kinds`.  tampers[k]: None, sig_bit, key_bit (that
    input's own signature / key), amount (its spent output's amount +-1) or other_spk (one bit of
    the scriptPubKey of a non-v1 spent output other than k's own).  Every input is placed twice with
    the same per-input generator: Taproot signatures commit to every spent output, so the first
    pass fixes the outputs and the second signs the final transaction.  Returns dict(t, inputs)."""
    import random
    n = len(kinds)
    tampers = tampers or [None] * n
    hash_types = hash_types or [rng.choice(S.HASH_TYPES) for _ in range(n)]
    t = S.s_tx(rng, nin=n)
    t["wit"] = None
    seeds = [rng.getrandbits(64) for _ in range(n)]
    inputs = []
    for _ in range(2):
        inputs = []
        for k, kind in enumerate(kinds):
            r2 = random.Random(seeds[k])
            own = tampers[k] if tampers[k] in ("sig_bit", "key_bit") else None
            if kind in V1_KINDS:
                inputs.append(v1_input(R, r2, t, k, kind, hash_types[k], own))
            else:
                inputs.append(ecdsa_input(R, O, r2, t, k, kind, own))
    for k, tam in enumerate(tampers):
        inputs[k]["tamper"] = tam
        sp = list(t["spent"])
        if tam == "amount":
            sp[k] = (sp[k][0] + rng.choice([1, -1]) if sp[k][0] > 0 else 1, sp[k][1])
        elif tam == "other_spk":
            others = [j for j in range(n) if j != k and kinds[j] not in V1_KINDS]
            if not others:
                inputs[k]["tamper"] = None
                continue
            j = rng.choice(others)
            sp[j] = (sp[j][0], _flip(sp[j][1], rng, len(sp[j][1]) - 12, len(sp[j][1]) - 2))
            inputs[k]["tamper"] = f"other_spk:{j}"
        t["spent"] = sp
    return dict(t=t, inputs=inputs)


def label_mixed(R, m):
    """The labelled transaction: dict(tx, spent, tamper, inputs=[dict(kind, tamper, ret, detail)]).
    Non-v1 inputs: the reference's verify_script_with_amount at 0xE15 (its err must be 0).  v1
    inputs: label_s's rule over the reference's per-check answers on the final bytes."""
    t = m["t"]
    tx, spent = _bytes(t), G.ser_outs(t["spent"])
    out = []
    for k, i in enumerate(m["inputs"]):
        if i["kind"] in V1_KINDS:
            assert is_v1(t["spent"][k][1])
            c = dict(tx=tx, spent=spent, nin=k, checks=i["checks"], arith=i["arith"])
            ret, serr = S.label_s(R, c)
        else:
            assert not is_v1(t["spent"][k][1])
            ret, err = R.verify_script_with_amount(t["spent"][k][1], t["spent"][k][0], tx, k, ALL)
            assert err == 0, err
            serr = None
        out.append(dict(kind=i["kind"], tamper=i["tamper"], ret=ret, detail=serr))
    return dict(tx=tx, spent=spent, inputs=out, tamper=[i["tamper"] for i in out])


def random_mixed_txs(R, O, rng, n_inputs, weights=None, nin_range=(2, 4), tamper_rate=0.25):
    """Fresh labelled mixed transactions holding at least n_inputs inputs in all."""
    weights = weights or [1] * len(KINDS)
    out, total = [], 0
    while total < n_inputs:
        n = rng.randrange(nin_range[0], nin_range[1] + 1)
        kinds = rng.choices(KINDS, weights, k=n)
        tampers = [rng.choice(TAMPERS) if rng.random() < tamper_rate else None for _ in range(n)]
        out.append(label_mixed(R, build_mixed_tx(R, O, rng, kinds, tampers)))
        total += n
    return out


def items_of(cases):
    return [dict(tx=c["tx"], spent=c["spent"], nin=c["nin"]) for c in cases]
