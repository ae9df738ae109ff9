"""What the rule-entry tests share (test_block_rules_host.py on the device-less engine, where a
device round is the host evaluation behind the device seam; test_block_rules_gpu.py on
librbc_amd.so, where it is tx_rules_kernel, dup_input_kernel and block_rules_kernel): the cases,
each compared with tests/block_rules_model.py on both routes, the small-round threshold at 0 (every
round a device round) or above every batch (every round on the host).  The shapes are the smallest
at which each piece can go wrong; the two transactions and the blocks of a megabyte are built here
and not stored."""
import functools
import gzip
import json
import os
import random

import bitcoinconsensus_amd as B
import block_commit_checks as C
import block_model as BM
import block_rules_model as M
import sighash_model as SM

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "tx_check_cases.json.gz")
SEED = 20261022
FINAL, NULL = 0xffffffff, M.NULL_PREVOUT
HEIGHT, CUTOFF = 700000, 1600000000
ALL = M.SEGWIT_ACTIVE | M.BIP34_ACTIVE
settings, routes, has_kernels = C.settings, C.routes, C.has_kernels


def bind(L):
    L = C.bind(L)
    B._bind_block_rules(L)
    return L


# ------------------------------------------------------------------------------------------------
# builders


def prev(k, n=0):
    """A distinct, non-null outpoint."""
    return (0x1000 + k).to_bytes(32, "little") + n.to_bytes(4, "little")


def out(value, script=b"\x51"):
    return value.to_bytes(8, "little", signed=True) + SM.cs(len(script)) + script


def tx(vin, vout, lock=0, witness=None, counts=None):
    """vin: [(outpoint36, scriptSig, sequence)].  counts=(k_in, k_out): the width in bytes (1, 3 or
    5) of the two CompactSize counts, canonical or not."""
    vin = [(p, s, q.to_bytes(4, "little")) for p, s, q in vin]
    raw = SM.ser_tx(b"\x02\0\0\0", vin, vout, lock.to_bytes(4, "little"), witness)
    if counts:
        assert witness is None and len(vin) < 253 and len(vout) < 253
        wide = lambda n, w: {1: bytes([n]), 3: b"\xfd" + n.to_bytes(2, "little"),
                             5: b"\xfe" + n.to_bytes(4, "little")}[w]
        ins = b"".join(p + SM.cs(len(s)) + s + q for p, s, q in vin)
        raw = b"\x02\0\0\0" + wide(len(vin), counts[0]) + ins + wide(len(vout), counts[1]) + \
            b"".join(vout) + lock.to_bytes(4, "little")
    return raw


def simple(k, lock=0, seq=FINAL, nin=1, value=1000):
    return tx([(prev(k, i), b"", seq) for i in range(nin)], [out(value)], lock)


def coinbase(script=None, height=HEIGHT, outs=None, witness=None, lock=0, seq=FINAL):
    script = M.push_int(height) + b"\x00" if script is None else script
    return tx([(NULL, script, seq)], [out(50 * 10 ** 8)] if outs is None else outs, lock, witness)


def sized(stripped, k=0, witness=None):
    """A transaction of exactly `stripped` bytes without its witness data: one output script of zero
    bytes is the filler."""
    base = len(tx([(prev(k), b"", FINAL)], [out(1, b"")]))
    pad = stripped - base
    pad -= SM.cs_len(pad) - 1
    t = tx([(prev(k), b"", FINAL)], [out(1, bytes(pad))], witness=witness)
    assert M.parse(t)["stripped_size"] == stripped
    return t


def block(txs, root=None, seed=0):
    return BM.make_block(random.Random(SEED + seed), txs, root)


def segwit_block(rest, nonce=None, commit="ok", cb_kw=None, filler=None):
    """A block whose coinbase commits to the witness tree of `rest`.  commit: "ok", "bad" or None;
    nonce: the coinbase's witness stack (default one 32-byte item); filler: (weight wanted): the
    last transaction gets one more witness item sized so that the block weighs exactly that."""
    def build(rest):
        stack = [bytes(range(32))] if nonce is None else nonce
        wroot = BM.merkle_root([BM.ZERO] + [BM.Tx(t).wtxid() for t in rest])[0]
        good = BM.sha256d(wroot + stack[0]) if stack and len(stack[0]) == 32 else bytes(32)
        outs = [out(50 * 10 ** 8)]
        if commit is not None:
            outs.append(BM.commit_out(good if commit == "ok" else bytes([good[0] ^ 1]) + good[1:]))
        return block([coinbase(outs=outs, witness=[stack] if stack is not None else None, **(cb_kw or {}))]
                     + rest)
    if filler is None:
        return build(rest)
    spend = lambda n: tx([(prev(9000), b"", FINAL)], [out(1)], witness=[[bytes(n)]])
    have = M.block_result(build(rest + [spend(70000)]), HEIGHT, CUTOFF, ALL)["weight"]
    raw = build(rest + [spend(70000 + filler - have)])  # (the item's length stays a 5-byte count)
    assert M.block_result(raw, HEIGHT, CUTOFF, ALL)["weight"] == filler
    return raw


# ------------------------------------------------------------------------------------------------
# transactions


@functools.lru_cache(maxsize=None)
def fixture():
    with gzip.open(FIXTURE) as f:
        return json.load(f)["cases"]


CHECKSIG, CHECKSIGVERIFY, MULTISIG, MULTISIGVERIFY = b"\xac", b"\xad", b"\xae", b"\xaf"


def script_cases():
    """(label, script, sigops): GetSigOpCount(false) at every edge of GetScriptOp."""
    s = [("empty", b"", 0)]
    for name, op, n in (("CHECKSIG", CHECKSIG, 1), ("CHECKSIGVERIFY", CHECKSIGVERIFY, 1),
                        ("CHECKMULTISIG", MULTISIG, 20), ("CHECKMULTISIGVERIFY", MULTISIGVERIFY, 20)):
        s.append((name, op, n))
        s.append((name + " x3 between other opcodes", b"\x76" + op + b"\x87" + op + op + b"\xb0", 3 * n))
    s.append(("inside a direct push", b"\x03\xac\xac\xac\xac", 1))
    s.append(("ends inside a direct push", b"\xac\x05\xac\xac", 1))
    s.append(("direct push of exactly the rest", b"\x02\xac\xac", 0))
    for op, w in ((0x4c, 1), (0x4d, 2), (0x4e, 4)):
        name = f"PUSHDATA{w}"
        s.append((name + " body skipped", bytes([op]) + (3).to_bytes(w, "little") + b"\xac" * 3 + b"\xac", 1))
        s.append((name + " ends in its length", b"\xac" + bytes([op]) + b"\xac" * (w - 1), 1))
        s.append((name + " ends in its body", b"\xae" + bytes([op]) + (4).to_bytes(w, "little") + b"\xac" * 3, 20))
        s.append((name + " with no length at all", b"\xac" + bytes([op]), 1))
        s.append((name + " of zero bytes", bytes([op]) + bytes(w) + b"\xac", 1))
    s.append(("PUSHDATA4 of 0xffffffff", b"\xac\x4e\xff\xff\xff\xff\xac\xac\xac", 1))
    s.append(("PUSHDATA4 of 0xfffffffc", b"\x4e\xfc\xff\xff\xff" + b"\xac" * 8, 0))
    s.append(("PUSHDATA2 of 300", b"\x4d\x2c\x01" + b"\xac" * 300 + b"\xaf", 20))
    for label, script, n in s:
        assert M.script_sigops(script) == n, label
    return s


@functools.lru_cache(maxsize=None)
def tx_cases():
    """[(label, raw)]: every case the model decides; the expected result is the model's."""
    rng = random.Random(SEED)
    c = [("fixture " + r["source"] + f" {k}", bytes.fromhex(r["tx"])) for k, r in enumerate(fixture())]
    MM = M.MAX_MONEY
    for v in (-1, 0, MM, MM + 1, -(1 << 63), (1 << 63) - 1):
        c.append((f"value {v}", tx([(prev(1), b"", FINAL)], [out(v)])))
    for a, b in ((MM - 5, 5), (MM - 5, 6), (MM, 0), (MM, 1), (1, MM), (MM, MM)):
        c.append((f"values {a} + {b}", tx([(prev(2), b"", FINAL)], [out(a), out(b)])))
    # 2^63 - 1 + 2^63 - 1 + 2: wraps 64 bits to zero when nothing is tested per output
    c.append(("a sum that would wrap", tx([(prev(3), b"", FINAL)], [out((1 << 63) - 1), out((1 << 63) - 1), out(2)])))
    c.append(("too large, then negative", tx([(prev(3), b"", FINAL)], [out(MM + 1), out(-1)])))
    c.append(("negative after a total that is too large", tx([(prev(3), b"", FINAL)], [out(MM), out(1), out(-1)])))
    for n in (0, 1, 2, 100, 101):
        c.append((f"coinbase scriptSig of {n}", coinbase(script=bytes([0x51]) * n)))
    c.append(("coinbase shape with two inputs", tx([(NULL, b"\x51\x51", FINAL), (prev(4), b"", FINAL)], [out(1)])))
    for at in (0, 1, 2):
        vin = [(NULL if k == at else prev(5, k), b"", FINAL) for k in range(3)]
        c.append((f"null prevout at {at} of 3", tx(vin, [out(1)])))
    c.append(("null hash, n = 0", tx([(bytes(36), b"\x51\x51", FINAL)], [out(1)])))
    c.append(("same hash, different n", tx([(prev(6, 0), b"", FINAL), (prev(6, 1), b"", FINAL)], [out(1)])))
    c.append(("no inputs, no outputs", b"\x02\0\0\0\x00\x00" + bytes(4)))
    c.append(("no outputs", tx([(prev(7), b"", FINAL)], [])))
    c.append(("no outputs, witness", tx([(prev(7), b"", FINAL)], [], witness=[[b"\x01"]])))
    for label, script, _ in script_cases():
        c.append(("scriptSig: " + label, tx([(prev(8), script, 5)], [out(1)], lock=7)))
        c.append(("scriptPubKey: " + label, tx([(prev(8), b"", FINAL)], [out(1, script)])))
    c.append(("sigops in both and in the coinbase", coinbase(script=b"\x51\xac\xae", outs=[out(1, b"\xac"), out(2, b"\xaf\xad")])))
    c.append(("sigops in witness items", tx([(prev(9), b"\xac", FINAL)], [out(1, b"\xae")], witness=[[b"\xac\xae" * 9, b"\xaf"]])))
    for ki in (1, 3, 5):
        for ko in (1, 3, 5):
            c.append((f"CompactSize widths {ki}, {ko}", tx([(prev(10), b"\xac", FINAL)], [out(1)], counts=(ki, ko))))
    c.append(("253 inputs, 254 outputs", tx([(prev(11, k), b"", k) for k in range(253)], [out(k) for k in range(254)])))
    c.append(("scriptSig of 253 bytes", tx([(prev(12), b"\x4c\xfa" + b"\xac" * 250 + b"\xac", FINAL)], [out(1)])))
    for k in range(8):  # whatever the blob holds before it, at each alignment
        c.append((f"after {k} odd bytes", tx([(prev(13), bytes(k), FINAL)], [out(1, b"\xac")], witness=[[b"\x07"]] if k & 1 else None)))
        c.append((f"aligned probe {k}", tx([(prev(14, 0), b"\xac", FINAL), (prev(14, 0), b"", 3)], [out(MM), out(0, b"\xae")], lock=k)))
    c += [(f"random {k}", SM.rand_tx(rng, 1 + k % 5, (25, 23, 1)[:1 + k % 3], sig_lens=[k % 7 * 15] * (1 + k % 5),
                                     witness=bool(k & 1))) for k in range(40)]
    c.append(("trailing byte", simple(15) + b"\x00"))
    c.append(("truncated", simple(15)[:-1]))
    c.append(("empty", b""))
    c.append(("witness flag, no inputs", b"\x02\0\0\0\x00\x01\x00\x01" + out(1) + bytes(4)))
    return c


def compare_txs(got, raws, labels):
    bad = [(lab, g, M.tx_result(r)) for g, r, lab in zip(got, raws, labels) if g != M.tx_result(r)]
    assert not bad, bad[:5]


def check_fixture_pins():
    """The fixture against the reference's own files: every tx_valid.json transaction passes, and
    the rows under "Tests for CheckTransaction()" fail as their comments say, in order; and the
    stored results are the model's."""
    rows = fixture()
    assert sum(r["source"] == "tx_valid.json" for r in rows) == 120 and len(rows) == 212
    assert all(r["result"]["status"] == M.TX_OK for r in rows if r["source"] == "tx_valid.json")
    assert [r["result"]["status"] for r in rows if r["check_transaction_section"]] == [
        M.VOUT_EMPTY, M.VOUT_NEGATIVE, M.VOUT_TOOLARGE, M.TXOUTTOTAL_TOOLARGE, M.INPUTS_DUPLICATE,
        M.CB_LENGTH, M.CB_LENGTH, M.PREVOUT_NULL, M.PREVOUT_NULL]
    sizes = [r["result"]["n_in"] == 1 and len(M.parse(bytes.fromhex(r["tx"]))["vin"][0][1])
             for r in rows if r["result"]["status"] == M.CB_LENGTH]
    assert sizes == [1, 101]
    for r in rows:
        assert M.tx_result(bytes.fromhex(r["tx"])) == r["result"]


def check_txs(L):
    L = bind(L)
    cases = tx_cases()
    labels, raws = [c[0] for c in cases], [c[1] for c in cases]
    want = [M.tx_result(r) for r in raws]
    assert {w["status"] for w in want} >= set(range(16, 25)) - {M.OVERSIZE} | {0, M.ERR_TX_DESERIALIZE, M.ERR_TX_SIZE_MISMATCH}
    for route, kw in routes(L):
        with settings(L, **kw):
            got = B.tx_check_batch(raws, library=L)
            st = B.last_block_stats(library=L)
            compare_txs(got, raws, labels)
            C.expect_route(st, route, rounds=1)
            assert st["txs"] == sum(w["status"] not in (2, 3) for w in want)
            for i in (0, len(raws) // 2, len(raws) - 4):
                assert B.tx_check_batch([raws[i]], library=L) == [got[i]]
            assert B.tx_check_batch([], library=L) == []
        with settings(L, block_round=7, **kw):  # cuts through the batch
            assert B.tx_check_batch(raws, library=L) == got
        with settings(L, txhash_blocks=0, **kw):  # no transaction is the host's
            assert B.tx_check_batch(raws, library=L) == got
        with settings(L, txhash_blocks=1, **kw):  # almost every transaction is
            assert B.tx_check_batch(raws, library=L) == got
    f = L.bcc_tx_check_batch
    res = (B.TxCheckResult * 1)()
    arr = (B.TxRef * 1)(B.TxRef(b"\0" * 10, 10))
    assert f(None, 1, res, 0) == -1 and f(arr, 1, None, 0) == -1 and f(None, 0, None, 0) == 0


def check_megabyte_txs(L):
    """1,000,000 stripped bytes pass, 1,000,001 are oversize, with and without witness data on top;
    on the device route with the long-chain threshold off, one lane walks the megabyte."""
    L = bind(L)
    a, b = sized(1000000), sized(1000001)
    w = sized(1000000, witness=[[bytes(50)]])
    raws = [simple(1), a, simple(2), b, w]
    want = [M.tx_result(r) for r in raws]
    assert [x["status"] for x in want] == [0, 0, 0, M.OVERSIZE, 0] and want[4]["stripped_size"] == 1000000
    for route, kw in routes(L):
        for th in (C.DEFAULT_TXHASH_BLOCKS, 0):
            with settings(L, txhash_blocks=th, **kw):
                assert B.tx_check_batch(raws, library=L) == want, (route, th)


# ------------------------------------------------------------------------------------------------
# duplicate inputs


def dup_tx(n, pair, k=0):
    """n inputs; pair = (i, j): input j repeats input i's outpoint; None: all distinct."""
    pts = [prev(100 + k, i) for i in range(n)]
    if pair:
        pts[pair[1]] = pts[pair[0]]
    return tx([(p, bytes([i % 5]) * (i % 3), FINAL) for i, p in enumerate(pts)], [out(1)])


def colliding(L, row, log2, slot, count, tag):
    """`count` distinct outpoints that start probing at `slot` for the transaction at `row`."""
    found, k = [], 0
    while len(found) < count:
        p = prev(50000 + tag, k)
        if B.debug_outpoint_slot(row, p, log2, library=L) == slot:
            found.append(p)
        k += 1
    return found


def check_duplicates(L):
    L = bind(L)
    cases = []
    for n in (2, 3, 64, 65):
        for pair in ((0, n - 1), (n // 2 - 1, n // 2) if n > 2 else (0, 1), None):
            cases.append((f"{n} inputs, pair {pair}", dup_tx(n, pair, k=n)))
    cases.append(("three equal", tx([(prev(1), b"", FINAL)] * 3, [out(1)])))
    # the same outpoint in two transactions, and once more inside a third
    cases.append(("shared with the next", simple(77, nin=2)))
    cases.append(("shared with the previous", simple(77, nin=2)))
    cases.append(("one input, the same outpoint", simple(77)))
    raws = [r for _, r in cases]
    want = [M.tx_result(r) for r in raws]
    assert [w["status"] for w in want[-3:]] == [0, 0, 0]
    assert sum(w["status"] == M.INPUTS_DUPLICATE for w in want) == 9
    for route, kw in routes(L):
        with settings(L, **kw):
            compare_txs(B.tx_check_batch(raws, library=L), raws, [c[0] for c in cases])
            compare_txs(B.tx_check_batch(raws[::-1], library=L), raws[::-1], [c[0] for c in cases][::-1])
    # chosen slots: the round is [one input, the probe]: the probe is row 1 of the round and its
    # inputs are the table's only rows
    for n_in, label in ((4, "chain"), (4, "wrap"), (2, "minimum table")):
        log2 = B.debug_dup_table_log2(n_in, library=L)
        assert 1 << log2 == {4: 8, 2: 4}[n_in]
        slot = (1 << log2) - 1 if label == "wrap" else 2
        for dup in (True, False):
            pts = colliding(L, 1, log2, slot, n_in, tag=len(label))
            if dup:
                pts[-1] = pts[-2]
            probe = tx([(p, b"", FINAL) for p in pts], [out(1)])
            want = M.tx_result(probe)
            assert want["status"] == (M.INPUTS_DUPLICATE if dup else 0)
            for route, kw in routes(L):
                with settings(L, **kw):
                    got = B.tx_check_batch([simple(1), probe], library=L)
                    assert got == [M.tx_result(simple(1)), want], (label, dup, route)
    # a transaction above the long-chain threshold: the host evaluates it during a device round
    for dup in (True, False):
        pts = [prev(300, 0), prev(300, 0 if dup else 1)]
        long = tx([(pts[0], bytes(1500), FINAL), (pts[1], b"", FINAL)], [out(1)])
        raws = [dup_tx(3, (0, 2)), long, dup_tx(3, None)]
        for route, kw in routes(L):
            with settings(L, **kw):
                got = B.tx_check_batch(raws, library=L)
                st = B.last_block_stats(library=L)
            compare_txs(got, raws, ["short", "long", "short"])
            assert got[1]["status"] == (M.INPUTS_DUPLICATE if dup else 0)
            assert st["host_long_txs"] == (1 if route == "device" and has_kernels(L) else 0), st


# ------------------------------------------------------------------------------------------------
# blocks


def plain_block(n=3, cb=None, txs=None, **kw):
    return block([coinbase() if cb is None else cb] + (txs if txs is not None else [simple(k) for k in range(1, n)]), **kw)


def sigop_block(extra):
    """20,000 sigops in one output script of 1,000 CHECKMULTISIG, plus `extra` CHECKSIG."""
    heavy = tx([(prev(1), b"", FINAL)], [out(1, MULTISIG * 1000)])
    return plain_block(txs=[heavy, tx([(prev(2), CHECKSIG * extra, FINAL)], [out(1)])])


def bad_tx(k=50):
    return tx([(prev(k), b"", FINAL)], [out(-1)])


@functools.lru_cache(maxsize=None)
def block_cases():
    """[(label, raw, height, cutoff, flags, status or None)]: one of each status with every earlier
    rule passing, pairs that pin the order, and the boundaries."""
    c = []
    add = lambda label, raw, status=None, height=HEIGHT, cutoff=CUTOFF, flags=ALL: \
        c.append((label, raw, height, cutoff, flags, status))
    ok = plain_block(5)
    add("ok", ok, 0)
    add("coinbase alone", plain_block(1), 0)
    add("truncated", ok[:-3], BM.ERR_DESERIALIZE)
    add("zero count", ok[:80] + b"\x00", BM.ERR_EMPTY)
    add("wrong root", plain_block(4, root=bytes(range(32))), BM.ERR_MERKLE_ROOT)
    t = [coinbase(), simple(1), simple(2)]
    add("mutated", block(t + [t[2]], root=BM.merkle_root([BM.Tx(x).txid() for x in t])[0]), BM.ERR_DUPLICATE)
    fill = lambda total, first=coinbase(): sized(total - 80 - 1 - len(first), k=3)
    add("stripped size 1,000,000", plain_block(txs=[fill(1000000)]), 0)
    add("stripped size 1,000,001", plain_block(txs=[fill(1000001)]), M.ERR_LENGTH)
    add("merkle before length", plain_block(txs=[fill(1000001)], root=bytes(32)), BM.ERR_MERKLE_ROOT)
    add("length before cb-missing", block([simple(1), fill(1000001, simple(1))]), M.ERR_LENGTH)
    add("no coinbase", block([simple(1), simple(2)]), M.ERR_CB_MISSING)
    add("coinbase second", block([simple(1), coinbase()]), M.ERR_CB_MISSING)
    add("cb-missing before a tx error", block([simple(1), bad_tx()]), M.ERR_CB_MISSING)
    add("two coinbases", plain_block(txs=[simple(1), coinbase(script=b"\x51\x52"), simple(2)]), M.ERR_CB_MULTIPLE)
    add("cb-multiple before a tx error", plain_block(txs=[bad_tx(), coinbase(script=b"\x51\x52")]), M.ERR_CB_MULTIPLE)
    ten = [simple(k) for k in range(1, 12)]
    both = list(ten)
    both[4], both[8] = tx([(prev(60), b"", FINAL)] * 2, [out(1)]), bad_tx()
    add("tx 5 before tx 9", plain_block(txs=both), M.ERR_TX)
    heavy = tx([(prev(61), b"", FINAL)], [out(1, MULTISIG * 1001)])
    add("tx error before sigops", plain_block(txs=[heavy] + both[1:]), M.ERR_TX)
    add("coinbase with a bad length", plain_block(cb=coinbase(script=b"\x51")), M.ERR_TX)
    for code, bad in ((M.VOUT_EMPTY, tx([(prev(62), b"", FINAL)], [])),
                      (M.VOUT_TOOLARGE, tx([(prev(62), b"", FINAL)], [out(M.MAX_MONEY + 1)])),
                      (M.TXOUTTOTAL_TOOLARGE, tx([(prev(62), b"", FINAL)], [out(M.MAX_MONEY), out(1)])),
                      (M.PREVOUT_NULL, tx([(prev(62), b"", FINAL), (NULL, b"", FINAL)], [out(1)]))):
        add(f"tx error {code}", plain_block(txs=[simple(1), bad, simple(2)]), M.ERR_TX)
    add("20,000 sigops", sigop_block(0), 0)
    add("20,001 sigops", sigop_block(1), M.ERR_SIGOPS)
    add("sigops before nonfinal", plain_block(txs=[heavy, simple(1, lock=HEIGHT, seq=0)]), M.ERR_SIGOPS)
    for lock in (0, HEIGHT - 1, HEIGHT, 499999999, 500000000, CUTOFF - 1, CUTOFF, 0xffffffff):
        for cutoff in (CUTOFF, CUTOFF + 1) if lock >= 500000000 else (CUTOFF,):
            final = lock == 0 or lock < (HEIGHT if lock < 500000000 else cutoff)
            add(f"lock time {lock} against {cutoff}", plain_block(txs=[simple(1), simple(2, lock=lock, seq=0)]),
                0 if final else M.ERR_NONFINAL, cutoff=cutoff)
    add("lock time above a small height", plain_block(txs=[simple(1, lock=3, seq=1)], cb=coinbase(height=3)),
        M.ERR_NONFINAL, height=3)
    add("non-final lock time, final sequences", plain_block(txs=[simple(1, lock=HEIGHT + 5, nin=3)]), 0)
    add("one sequence of three not final", plain_block(txs=[tx(
        [(prev(63, 0), b"", FINAL), (prev(63, 1), b"", FINAL - 1), (prev(63, 2), b"", FINAL)], [out(1)], lock=HEIGHT)]),
        M.ERR_NONFINAL)
    add("non-final coinbase", plain_block(cb=coinbase(lock=HEIGHT, seq=0)), M.ERR_NONFINAL)
    add("a negative cutoff", plain_block(txs=[simple(1, lock=500000000, seq=0)]), M.ERR_NONFINAL, cutoff=-1)
    add("nonfinal before cb-height", plain_block(cb=coinbase(height=HEIGHT + 1), txs=[simple(1, lock=HEIGHT, seq=0)]),
        M.ERR_NONFINAL)
    for h in (0, 1, 16, 17, 127, 128, 32767, 32768, (1 << 31) - 1):
        want = M.push_int(h)
        add(f"height {h}", plain_block(cb=coinbase(height=h)), 0, height=h)
        add(f"height {h}, exactly the prefix", plain_block(cb=coinbase(script=want + b"\x00" * (len(want) < 2))), 0, height=h)
        add(f"height {h}, one byte short", plain_block(cb=coinbase(script=want[:-1])), None, height=h)
        add(f"height {h}, last byte wrong", plain_block(cb=coinbase(script=want[:-1] + bytes([want[-1] ^ 1]) + b"\x51")),
            M.ERR_CB_HEIGHT, height=h)
        wide = h.to_bytes(max(1, (h.bit_length() + 8) // 8) + (h > 16), "little")
        add(f"height {h}, not minimal", plain_block(cb=coinbase(script=bytes([len(wide)]) + wide)), M.ERR_CB_HEIGHT, height=h)
        add(f"height {h}, BIP34 off", plain_block(cb=coinbase(script=b"\x51\x51")), 0, height=h, flags=M.SEGWIT_ACTIVE)
        add(f"height {h}, the next one's", plain_block(cb=coinbase(height=h + 1 if h < (1 << 31) - 1 else h - 1)),
            M.ERR_CB_HEIGHT, height=h)
    wtx = lambda k: tx([(prev(70 + k), b"", FINAL)], [out(1)], witness=[[bytes([k]) * 40]])
    add("witness commitment", segwit_block([wtx(1), simple(2), wtx(3)]), 0)
    add("bad reserved value", segwit_block([wtx(1)], nonce=[bytes(31)]), BM.ERR_WITNESS_NONCE_SIZE)
    add("commitment mismatch", segwit_block([wtx(1), wtx(2)], commit="bad"), BM.ERR_WITNESS_MERKLE)
    add("unexpected witness", segwit_block([wtx(1)], commit=None), BM.ERR_UNEXPECTED_WITNESS)
    add("segwit off, witness data", segwit_block([wtx(1)]), BM.ERR_UNEXPECTED_WITNESS, flags=M.BIP34_ACTIVE)
    add("cb-height before the commitment", segwit_block([wtx(1)], commit="bad", cb_kw=dict(height=5)), M.ERR_CB_HEIGHT)
    add("weight 4,000,000", segwit_block([wtx(1)], filler=4000000), 0)
    add("weight 4,000,001", segwit_block([wtx(1)], filler=4000001), M.ERR_WEIGHT)
    add("witness status before weight", segwit_block([wtx(1)], commit="bad", filler=4000001), BM.ERR_WITNESS_MERKLE)
    for label, raw, height, cutoff, flags, status in c:
        got = M.block_result(raw, height, cutoff, flags)
        assert status is None or got["status"] == status, (label, got["status"], status)
    assert {M.block_result(r, h, t, f)["status"] for _, r, h, t, f, _ in c} == set(range(16))
    return c


@functools.lru_cache(maxsize=None)
def small_blocks(n=65):
    """n small blocks of 1..9 transactions with every status a small block can have."""
    small = [x for x in block_cases() if len(x[1]) < 4000]
    return [small[(7 * k) % len(small)] for k in range(n)]


def args_of(cases):
    return [(raw, h, t, f) for _, raw, h, t, f, _ in cases]


def compare_blocks(L, got, cases):
    for g, (label, raw, h, t, f, _) in zip(got, cases):
        want = M.block_result(raw, h, t, f)
        assert g == want, (label, {k: (g[k], want[k]) for k in g if g[k] != want[k]})
    # the commitment fields are bcc_block_commitments_batch's on the same bytes
    com = B.block_commitments([(raw, f & M.SEGWIT_ACTIVE) for _, raw, _, _, f, _ in cases], txids=False, library=L)
    for g, c, (label, *_) in zip(got, com, cases):
        for k in ("n_tx", "commit_pos", "merkle_root", "witness_root"):
            assert g[k] == c[k], (label, k)
        if c["status"] in (1, 2, 3, 4):
            assert g["status"] == c["status"], label


def check_blocks(L):
    L = bind(L)
    cases = [x for x in block_cases() if len(x[1]) < 500000]
    for route, kw in routes(L):
        with settings(L, **kw):
            got = B.block_check_batch(args_of(cases), library=L)
            st = B.last_block_stats(library=L)
            compare_blocks(L, got, cases)
            assert st["blocks"] == len(cases)
            for i in (0, 2, 9, len(cases) - 1):
                assert B.block_check_batch(args_of(cases[i:i + 1]), library=L) == [got[i]], cases[i][0]
    f = L.bcc_block_check_batch
    res = (B.BlockCheckResult * 1)()
    arr = (B.BlockCheckRef * 1)(B.BlockCheckRef(None, 0, 0, 0, 0))
    assert f(None, 1, res, 0) == -1 and f(arr, 1, None, 0) == -1 and f(arr, 1, res, 0) == -1
    assert f(None, 0, None, 0) == 0


def check_megabyte_blocks(L):
    """The blocks at the size and weight limits (1 MB of stripped bytes, 4 MB of weight)."""
    L = bind(L)
    cases = [x for x in block_cases() if len(x[1]) >= 500000]
    assert len(cases) == 7
    for route, kw in routes(L):
        with settings(L, **kw):
            compare_blocks(L, B.block_check_batch(args_of(cases), library=L), cases)


def check_batches_and_cuts(L, set_devices):
    """Batches of 1, 63, 64 and 65 blocks, round cuts of 7 and 64 transactions, a two-entry device
    list: always the single call's results."""
    L = bind(L)
    cases = small_blocks()
    for route, kw in routes(L):
        with settings(L, **kw):
            whole = B.block_check_batch(args_of(cases), library=L)
            C.expect_route(B.last_block_stats(library=L), route, rounds=1)
            compare_blocks(L, whole, cases)
            for n in (1, 63, 64):
                assert B.block_check_batch(args_of(cases[:n]), library=L) == whole[:n]
        for cut in (7, 64):
            with settings(L, block_round=cut, **kw):
                assert B.block_check_batch(args_of(cases), library=L) == whole
                st = B.last_block_stats(library=L)
                assert st["device_rounds"] + st["host_rounds"] > (1 if cut == 64 else 10), st
        set_devices([0, 0])
        try:
            with settings(L, **kw):
                many = cases * 8  # enough transactions for two shares
                assert B.block_check_batch(args_of(many), device=-1, library=L) == whole * 8
                st = B.last_block_stats(library=L)
                assert st["device_rounds"] + st["host_rounds"] == 2, st
        finally:
            set_devices([0])


def fault_sequence(library=None):
    """bcc_debug_fail_device_rounds against the rule entries' rounds: one fault is retried, two
    fall back to the host, a sticky code goes straight to the host, BCC_DEVICE_FAILURE_ERROR
    returns -1; every delivered result is the model's."""
    cases = small_blocks()
    raws = [r for _, r in tx_cases()[200:330]]
    want_tx = [M.tx_result(r) for r in raws]
    with settings(library) as L:
        L = bind(L)
        want = B.block_check_batch(args_of(cases), library=L)
        compare_blocks(L, want, cases)

        def run_blocks():
            assert B.block_check_batch(args_of(cases), library=L) == want

        def run_txs():
            assert B.tx_check_batch(raws, library=L) == want_tx

        for run in (run_blocks, run_txs):
            for inject, retries, host_rounds in (
                    (lambda: None, 0, 0),
                    (lambda: L.bcc_debug_fail_device_rounds(1), 1, 0),
                    (lambda: L.bcc_debug_fail_device_rounds(2), 1, 1),
                    (lambda: L.bcc_debug_fail_device_rounds_code(1, C.LAUNCH_FAILURE), 0, 1)):
                before = L.bcc_host_fallback_rounds()
                inject()
                try:
                    run()
                finally:
                    L.bcc_debug_fail_device_rounds(0)
                st = B.last_block_stats(library=L)
                assert (st["device_retries"], st["host_rounds"]) == (retries, host_rounds), (run.__name__, st)
                assert st["device_rounds"] == 1 - host_rounds, (run.__name__, st)
                assert L.bcc_host_fallback_rounds() - before == host_rounds
            L.bcc_set_device_failure_policy(B.DEVICE_FAILURE_ERROR)
            L.bcc_debug_fail_device_rounds(3)
            try:
                try:
                    run()
                    raise AssertionError("no error under BCC_DEVICE_FAILURE_ERROR")
                except RuntimeError:
                    pass
            finally:
                L.bcc_debug_fail_device_rounds(0)
                L.bcc_set_device_failure_policy(B.DEVICE_FAILURE_HOST)
            run()
            st = B.last_block_stats(library=L)
            assert (st["device_retries"], st["host_rounds"]) == (0, 0), st
    return True
