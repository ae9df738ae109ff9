"""Generate tests/golden/mixed_inputs.json.gz (run in the build container, where the reference exists).

    python3 tests/golden/make_mixed_inputs_fixtures.py

Inputs and the REFERENCE's recorded answers (oracle/_ref/libref_consensus.so) for
bcc_verify_inputs_batch (tests/mixed_input_cases.py):

  mixed                     transactions of 2-4 inputs that mix native v1 inputs (key path with every
                            hash type, script path from taproot_spend_cases' templates) with P2PKH,
                            P2WPKH, P2SH-P2WPKH, 2-of-3 P2WSH and legacy 2-of-3 P2SH inputs.  About
                            1 input in 4 is tampered (a signature bit, a key bit, its spent amount
                            +-1, the scriptPubKey of ANOTHER input's spent output) and every input of
                            the transaction is labelled after the tamper: non-v1 inputs by
                            verify_script_with_amount at 0xE15, v1 inputs by label_s's rule over
                            CheckSchnorrSignature's answers.
  taproot_spends_at_0xE15   verify_script_with_amount at 0xE15 (v1 unchecked) for every case of
                            taproot_spends.json.gz, in its order.
  contract_etx              the transaction error of the zero-input and the witness-marker
                            transaction of mixed_input_cases.contract_cases.

ECDSA signatures are the reference's (ref_sign) over the oracle's SignatureHash; Schnorr signatures
are the reference's over the sighash the reference computed."""
import gzip
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mixed_input_cases as M  # noqa: E402
import taproot_spend_cases as S  # noqa: E402
from oracle_ctypes import Oracle, Reference  # noqa: E402


def plan(rng):
    """[(kinds, tampers, hash_types)]: 48 transactions; every kind, hash type and tamper occurs."""
    out = []
    hts = 0
    for k in range(48):
        n = 2 + k % 3
        if k % 4 == 3:  # one quarter is not mixed: all v1 or all non-v1
            kinds = [rng.choice(M.V1_KINDS if k % 8 == 3 else M.ECDSA_KINDS) for _ in range(n)]
        else:
            kinds = [M.V1_KINDS[((k + j) // 2) % 2] if j % 2 == k % 2 else M.ECDSA_KINDS[(k + j) % 5]
                     for j in range(n)]
        tampers = [None] * n
        if k % 6 != 2:  # 40 of 144 inputs, the four tampers in turn
            tampers[rng.randrange(n)] = M.TAMPERS[(k - (k + 3) // 6) % 4]
        ht = []
        for kind in kinds:
            ht.append(S.HASH_TYPES[hts % 7])
            hts += kind == "tr_key"
        out.append((kinds, tampers, ht))
    return out


def main():
    R, O = Reference(), Oracle()
    rng = random.Random(0x1A9075)
    txs = [M.label_mixed(R, M.build_mixed_tx(R, O, rng, kinds, tampers, hts))
           for kinds, tampers, hts in plan(rng)]
    ins = [i for t in txs for i in t["inputs"]]
    valid = sum(i["ret"] == 1 for i in ins)
    assert len(txs) >= 40 and all(2 <= len(t["inputs"]) <= 4 for t in txs)
    both = sum(1 for t in txs if len({i["kind"] in M.V1_KINDS for i in t["inputs"]}) == 2)
    assert 4 * both >= 3 * len(txs), both
    assert 0.3 * len(ins) <= valid <= 0.7 * len(ins), (valid, len(ins))
    for kind in M.KINDS:
        assert {i["ret"] for i in ins if i["kind"] == kind} == {0, 1}, kind
    tampered = sum(i["tamper"] is not None for i in ins)
    assert {(i["tamper"] or "").split(":")[0] for i in ins} >= set(M.TAMPERS)
    # only a mixed call can show this: another input's scriptPubKey changed, the Taproot inputs
    # that sign every spent output fail, an ECDSA input of the same transaction stays valid
    shown = 0
    for t in txs:
        if any((x or "").startswith("other_spk") for x in t["tamper"]):
            v1 = [i["ret"] for i in t["inputs"] if i["kind"] in M.V1_KINDS]
            ec = [i["ret"] for i in t["inputs"] if i["kind"] not in M.V1_KINDS]
            shown += 0 in v1 and 1 in ec
    assert shown >= 1, "no transaction shows the cross-kind effect"
    gold = S.load_golden()
    plain = []
    for c in gold:
        spk = S._spent_script(c["spent"], c["nin"])
        amount = int.from_bytes(_nth_out(c["spent"], c["nin"])[:8], "little", signed=True)
        plain.append(list(R.verify_script_with_amount(spk, amount, c["tx"], c["nin"], M.ALL)))
    doc = dict(source="oracle/_ref: ref_verify_script_with_amount (non-v1 inputs, flags 0xE15) and "
                      "ref_taproot_check under taproot_spend_cases.label_s (v1 inputs)",
               mixed=[dict(tx=t["tx"].hex(), spent=t["spent"].hex(), tamper=t["tamper"],
                           inputs=t["inputs"]) for t in txs],
               taproot_spends_at_0xE15=plain, contract_etx={})
    M._fixture = doc  # contract_cases takes its base transactions from the mixed ones
    for cse in M.contract_cases():
        if cse["expected"][1] is None:
            doc["contract_etx"][cse["cls"].split(":")[1]] = R.verify_script_with_amount(
                b"\x51", 0, cse["tx"], cse["nin"], M.ALL)[1]
    etx = doc["contract_etx"]
    with gzip.open(M.GOLDEN, "wt") as f:
        json.dump(doc, f, separators=(",", ":"))
    # the contract cases' transaction errors are the reference's
    M._fixture = None
    for c in M.all_contract_cases():
        if c["expected"][1] in (M.ERR_TX_INDEX, M.ERR_TX_SIZE_MISMATCH, M.ERR_TX_DESERIALIZE):
            got = R.verify_script_with_amount(b"\x51", 0, c["tx"], c["nin"], M.ALL)
            assert got == (0, c["expected"][1]), (c["cls"], got)
    by = {}
    for i in ins:
        by.setdefault(i["kind"], [0, 0])[i["ret"]] += 1
    print(len(txs), "txs", len(ins), "inputs", valid, "valid", tampered, "tampered", both, "mixed txs",
          by, "etx", etx, os.path.getsize(M.GOLDEN), "bytes")
    assert os.path.getsize(M.GOLDEN) <= 200_000


def _nth_out(spent, nin):
    """The serialized CTxOut nin of a spent-outputs blob (short compact sizes)."""
    o = 1 if spent[0] < 253 else 3
    for k in range(nin + 1):
        ln = spent[o + 8]
        w = 1
        if ln == 253:
            ln, w = int.from_bytes(spent[o + 9:o + 11], "little"), 3
        if k == nin:
            return spent[o:o + 8 + w + ln]
        o += 8 + w + ln
    raise IndexError(nin)


if __name__ == "__main__":
    main()
