"""Signed spends over every ECDSA-era hash type, labelled by the reference (run where oracle/_ref
is built).

    python3 tests/golden/make_hashtype_spends.py

Transactions of 1 to 40 inputs whose inputs cycle through four spend kinds (P2PKH, P2SH 2-of-3
multisig, P2WPKH, P2WSH) and the hash types ALL, NONE, SINGLE and their ANYONECANPAY forms; output
counts below, at and above the input count put SIGHASH_SINGLE on both sides of its last valid
index.  Signatures are made by the reference's libsecp256k1 (Reference.sign) over
sighash_model.sighash of the transaction with empty scriptSigs.  About one item in ten is
mutated: the signature's hash type byte replaced, a bit of an output's value flipped, or a bit of
another input's nSequence flipped (a mutated item carries its own copy of the transaction);
whether that invalidates the spend depends on the hash type, and the reference decides: every
item's (ret, err) is what bitcoinconsensus_verify_script_with_amount of oracle/_ref returns under
`flags`.

Output: hashtype_spends.json.gz = {"flags", "txs": [hex], "items": [{"tx": index into txs, "nin",
"spk", "amount", "kind", "hashtype", "mutation", "tx_inputs", "ret", "err"}], "long_none": {"tx",
"items": [{"nin", "spk", "amount", "ret", "err"}]}}: long_none is one transaction of 200 P2PKH
inputs all signed with SIGHASH_NONE.  Data only; regenerates byte for byte.
"""
import gzip
import hashlib
import json
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sighash_model as M  # noqa: E402
from oracle_ctypes import Reference  # noqa: E402
from script_asm import hash160, push_data, ser_tx  # noqa: E402

FLAGS = 0xE15  # every flag of the interface
HTS = (1, 2, 3, 0x81, 0x82, 0x83)
KINDS = ("p2pkh", "p2sh_multisig", "p2wpkh", "p2wsh")
SIZES = (1, 2, 3, 5, 8, 13, 21, 40, 1, 2, 4, 6, 10, 16, 30, 40, 7, 25, 40)
MUTATIONS = ("hashtype_byte", "output", "other_sequence")


def seckey(i):
    return hashlib.sha256(b"hashtype spends %d" % i).digest()


def main():
    R = Reference()
    pubs = {}

    def pub(i):
        if i not in pubs:
            pubs[i] = R.pubkey_create(seckey(i), True)
        return pubs[i]

    txs, items = [], []
    serial = 0
    for t, n in enumerate(SIZES):
        nout = (n, max(1, n - 1), n + 1, 1, n // 2 + 1)[t % 5]
        prev = [hashlib.sha256(b"hashtype prevout %d %d" % (t, k)).digest() + struct.pack("<I", k % 4)
                for k in range(n)]
        seqs = [(0xFFFFFFFF, 0xFFFFFFFE, 7 + k, 0)[(k + t) % 4] for k in range(n)]
        amounts = [100000 + 977 * k + t for k in range(n)]
        outs = [(40000 + 13 * j, (b"\x51", b"\x00\x14" + bytes([j]) * 20, b"")[j % 3])
                for j in range(nout)]
        unsigned = ser_tx(2, [(prev[k], b"", seqs[k]) for k in range(n)], outs, t)
        spks, sigs, wits, metas = [], [], [], []
        for k in range(n):
            kind = KINDS[(k + t) % 4]
            ht = HTS[(k // 4 + k + 2 * t) % 6]
            mutation = MUTATIONS[serial % 3] if serial % 10 == 3 else ""
            if mutation == "other_sequence" and n == 1:
                mutation = "output"
            byte = HTS[(HTS.index(ht) + 1 + serial % 5) % 6] if mutation == "hashtype_byte" else ht

            def sign(i, code, sv, ht=ht, byte=byte, k=k):
                m = M.sighash(unsigned, code, k, ht, amounts[k], sv)
                return R.sign(seckey(i), m) + bytes([byte])

            p = pub(serial)
            pkh = b"\x76\xa9\x14" + hash160(p) + b"\x88\xac"
            if kind == "p2pkh":
                spk, ss, wit = pkh, push_data(sign(serial, pkh, 0)) + push_data(p), []
            elif kind == "p2sh_multisig":
                keys = [pub(1000 * serial + j) for j in range(3)]
                redeem = b"\x52" + b"".join(push_data(x) for x in keys) + b"\x53\xae"
                spk = b"\xa9\x14" + hash160(redeem) + b"\x87"
                ss = b"\x00" + b"".join(push_data(sign(1000 * serial + j, redeem, 0))
                                        for j in (0, 2)) + push_data(redeem)
                wit = []
            elif kind == "p2wpkh":
                spk, ss, wit = b"\x00\x14" + hash160(p), b"", [sign(serial, pkh, 1), p]
            else:
                script = push_data(p) + b"\xac"
                spk = b"\x00\x20" + hashlib.sha256(script).digest()
                ss, wit = b"", [sign(serial, script, 1), script]
            spks.append(spk)
            sigs.append(ss)
            wits.append(wit)
            metas.append((kind, ht, mutation))
            serial += 1

        def final(seqs=seqs, outs=outs):
            return ser_tx(2, [(prev[k], sigs[k], seqs[k]) for k in range(n)], outs, t, wits)

        tx = final()
        for k in range(n):
            kind, ht, mutation = metas[k]
            raw = tx
            if mutation == "output":
                j = k if k < nout else 0
                o2 = list(outs)
                o2[j] = (outs[j][0] ^ (1 << (k % 16)), outs[j][1])
                raw = final(outs=o2)
            elif mutation == "other_sequence":
                s2 = list(seqs)
                s2[(k + 1) % n] ^= 1 << (k % 32)
                raw = final(seqs=s2)
            if raw.hex() not in txs:
                txs.append(raw.hex())
            ret, err = R.verify_script_with_amount(spks[k], amounts[k], raw, k, FLAGS)
            items.append(dict(tx=txs.index(raw.hex()), nin=k, spk=spks[k].hex(), amount=amounts[k],
                              kind=kind, hashtype=ht, mutation=mutation, tx_inputs=n, ret=ret,
                              err=int(err)))
    # one transaction of 200 P2PKH inputs, every one signed with NONE: its preimages are 129-block
    # chains, the ones bcc_set_host_chain_blocks sends to the host
    n = 200
    prev = [hashlib.sha256(b"hashtype long %d" % k).digest() + struct.pack("<I", k % 2)
            for k in range(n)]
    outs = [(50000, b"\x51"), (60000, b"\x00\x14" + bytes(20))]
    unsigned = ser_tx(1, [(prev[k], b"", 0xFFFFFFFD) for k in range(n)], outs, 0)
    lspk, lsig = [], []
    for k in range(n):
        p = pub(500000 + k)
        pkh = b"\x76\xa9\x14" + hash160(p) + b"\x88\xac"
        sig = R.sign(seckey(500000 + k), M.sighash(unsigned, pkh, k, 2, 0, 0)) + b"\x02"
        lspk.append(pkh)
        lsig.append(push_data(sig) + push_data(p))
    ltx = ser_tx(1, [(prev[k], lsig[k], 0xFFFFFFFD) for k in range(n)], outs, 0)
    long_items = []
    for k in range(n):
        ret, err = R.verify_script_with_amount(lspk[k], 70000 + k, ltx, k, FLAGS)
        long_items.append(dict(nin=k, spk=lspk[k].hex(), amount=70000 + k, ret=ret, err=int(err)))
    long_none = dict(tx=ltx.hex(), items=long_items)
    raw = json.dumps(dict(flags=FLAGS, txs=txs, items=items, long_none=long_none),
                     separators=(",", ":"),
                     sort_keys=True).encode()
    with open(os.path.join(HERE, "hashtype_spends.json.gz"), "wb") as fh:
        with gzip.GzipFile(fileobj=fh, mode="wb", mtime=0, filename="") as gz:
            gz.write(raw)
    hist = {}
    for it in items:
        key = (it["mutation"] or "plain", it["ret"])
        hist[key] = hist.get(key, 0) + 1
    assert all(it["ret"] == 1 for it in long_items)
    print(f"hashtype_spends: {len(items)} items, {len(txs)} txs, {sum(i['ret'] for i in items)} valid; "
          f"{sorted(hist.items())}")


if __name__ == "__main__":
    main()
