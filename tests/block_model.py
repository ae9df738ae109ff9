"""A hashlib model of what the block entries compute (include/bcc_amd.h bcc_tx_hashes_batch,
bcc_merkle_root, bcc_block_commitments_batch), and the cases the CPU and GPU suites share.

The model restates, independently of the engine: the serialization without marker, flag and
witnesses (primitives/transaction.h SerializeTransaction with fAllowWitness = false), SHA-256d,
ComputeMerkleRoot with its mutation flag (consensus/merkle.cpp:45-62) and the block rules of
CheckBlock / ContextualCheckBlock (validation.cpp:3364-3380, 3575-3610) with
GetWitnessCommitmentIndex (consensus/validation.h:161-179).  All hashes are raw digest bytes.
"""
import functools
import gzip
import hashlib
import json
import os
import random

import sighash_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "block_commit.json.gz")
SEED = 20261021

OK, ERR_DESERIALIZE, ERR_EMPTY, ERR_MERKLE_ROOT, ERR_DUPLICATE = 0, 1, 2, 3, 4
ERR_WITNESS_NONCE_SIZE, ERR_WITNESS_MERKLE, ERR_UNEXPECTED_WITNESS = 5, 6, 7
ERR_TX_SIZE_MISMATCH, ERR_TX_DESERIALIZE = 2, 3  # bitcoinconsensus.h
ZERO = bytes(32)
COMMIT_HEAD = bytes([0x6a, 0x24, 0xaa, 0x21, 0xa9, 0xed])


def sha256d(b):
    return hashlib.sha256(hashlib.sha256(b).digest()).digest()


# ------------------------------------------------------------------------------------------------
# transactions


def _compact(r):
    """ReadCompactSize with its range check (serialize.h:318-347)."""
    k = r.take(1)[0]
    if k < 253:
        return k
    v = int.from_bytes(r.take({253: 2, 254: 4, 255: 8}[k]), "little")
    if v < {253: 253, 254: 0x10000, 255: 1 << 32}[k] or v > 0x02000000:
        raise ValueError("non-canonical or oversized CompactSize")
    return v


class Tx:
    """A parsed transaction: the fields the rules read and the offsets the hashes need."""

    def __init__(self, raw, pos=0):
        r = M._Reader(raw)
        r.i = pos
        self.start = pos
        r.take(4)
        n = _compact(r)
        self.extended = False
        if n == 0:
            flag = r.take(1)[0]
            if flag != 0:
                if flag != 1:
                    raise ValueError("unknown optional data")
                self.extended = True
                n = _compact(r)
        self.vin_start = r.i
        for _ in range(n):
            r.take(36)
            r.take(_compact(r))
            r.take(4)
        self.n_in = n
        self.vout = []
        if n or self.extended:
            for _ in range(_compact(r)):
                r.take(8)
                self.vout.append(r.take(_compact(r)))
        self.wit_start = r.i
        self.witness = []
        if self.extended:
            for _ in range(n):
                self.witness.append([r.take(_compact(r)) for _ in range(_compact(r))])
            if not any(self.witness):
                raise ValueError("superfluous witness record")
        r.take(4)
        self.end = r.i
        self.raw = raw[pos:self.end]

    def stripped(self):
        if not self.extended:
            return self.raw
        return self.raw[:4] + self.raw[6:self.wit_start - self.start] + self.raw[-4:]

    def txid(self):
        return sha256d(self.stripped())

    def wtxid(self):
        return sha256d(self.raw)


def tx_hashes(raw):
    """(txid, wtxid, err) as bcc_tx_hashes_batch reports them for one item."""
    try:
        t = Tx(bytes(raw))
    except (ValueError, IndexError, KeyError):
        return ZERO, ZERO, ERR_TX_DESERIALIZE
    if t.end != len(raw):
        return ZERO, ZERO, ERR_TX_SIZE_MISMATCH
    return t.txid(), t.wtxid(), 0


# ------------------------------------------------------------------------------------------------
# merkle trees


def merkle_root(leaves):
    """ComputeMerkleRoot: (root, mutated)."""
    h = list(leaves)
    if not h:
        return ZERO, False
    mutated = False
    while len(h) > 1:
        for k in range(0, len(h) - 1, 2):
            if h[k] == h[k + 1]:
                mutated = True
        if len(h) & 1:
            h.append(h[-1])
        h = [sha256d(h[k] + h[k + 1]) for k in range(0, len(h), 2)]
    return h[0], mutated


# ------------------------------------------------------------------------------------------------
# blocks


def block_result(raw, segwit_active):
    """The bcc_block_result of one block, with its txids (None when the block gives none)."""
    bad = dict(status=ERR_DESERIALIZE, n_tx=0, commit_pos=-1, merkle_root=ZERO, witness_root=ZERO,
               txids=None)
    raw = bytes(raw)
    if len(raw) < 80:
        return bad
    try:
        r = M._Reader(raw)
        r.i = 80
        count = _compact(r)
        txs = []
        for _ in range(count):
            t = Tx(raw, r.i)
            r.i = t.end
            txs.append(t)
    except (ValueError, IndexError, KeyError):
        return bad
    if r.i != len(raw):
        return bad
    if not txs:
        return dict(bad, status=ERR_EMPTY)
    txids = [t.txid() for t in txs]
    root, mutated = merkle_root(txids)
    commit_pos = -1
    for o, spk in enumerate(txs[0].vout):
        if len(spk) >= 38 and spk[:6] == COMMIT_HEAD:
            commit_pos = o
    out = dict(status=OK, n_tx=len(txs), commit_pos=commit_pos, merkle_root=root, witness_root=ZERO,
               txids=txids)
    nonce_ok = False
    if segwit_active and commit_pos >= 0:
        w = txs[0].witness[0] if txs[0].n_in and txs[0].witness else []
        nonce_ok = len(w) == 1 and len(w[0]) == 32
        if nonce_ok:
            out["witness_root"] = merkle_root([ZERO] + [t.wtxid() for t in txs[1:]])[0]
    if root != raw[36:68]:
        out["status"] = ERR_MERKLE_ROOT
    elif mutated:
        out["status"] = ERR_DUPLICATE
    elif segwit_active and commit_pos >= 0:
        if not nonce_ok:
            out["status"] = ERR_WITNESS_NONCE_SIZE
        elif sha256d(out["witness_root"] + txs[0].witness[0][0]) != txs[0].vout[commit_pos][6:38]:
            out["status"] = ERR_WITNESS_MERKLE
    elif any(t.extended for t in txs):
        out["status"] = ERR_UNEXPECTED_WITNESS
    return out


# ------------------------------------------------------------------------------------------------
# case builders (seeded; the suites compare the engine with the model on these)


def padded_tx(rng, total_len=None, stripped_len=None, witness=False, nin=1, nout=1):
    """A transaction of random bytes whose full (total_len) or stripped (stripped_len)
    serialization has exactly the length asked for: the first scriptSig is the padding."""
    want = total_len if total_len is not None else stripped_len
    ends = [(rng.randbytes(36), rng.randbytes(4)) for _ in range(nin)]
    vout = [rng.randbytes(8) + M.cs(5) + rng.randbytes(5) for _ in range(nout)]
    wit = [[rng.randbytes(33)] for _ in range(nin)] if witness else None
    version, locktime, filler = rng.randbytes(4), rng.randbytes(4), rng.randbytes(want)
    for pad in range(want + 1):
        vin = [(p, filler[:pad] if k == 0 else b"", q) for k, (p, q) in enumerate(ends)]
        t = M.ser_tx(version, vin, vout, locktime, wit)
        got = len(t) if total_len is not None else len(Tx(t).stripped())
        if got == want:
            return t
        if got > want:
            break
    raise ValueError(f"no padding gives {want} bytes")


@functools.lru_cache(maxsize=None)
def tx_cases(seed=SEED):
    """[(label, raw)] for bcc_tx_hashes_batch: every length class the issue names."""
    rng = random.Random(seed)
    out = []
    for wit in (False, True):
        for m in (0, 1, 55, 56, 63):
            for base in (128, 320):
                out.append((f"full%64={m} wit={wit}", padded_tx(rng, total_len=base + m, witness=wit)))
                out.append((f"stripped%64={m} wit={wit}",
                            padded_tx(rng, stripped_len=base + m, witness=wit)))
        for k in range(64):  # the two range joins of a witness txid at every offset in a block
            out.append((f"sweep {k} wit={wit}", padded_tx(rng, total_len=200 + k, witness=wit)))
    out.append(("no outputs", padded_tx(rng, total_len=90, nout=0)))
    out.append(("no outputs, witness", padded_tx(rng, total_len=130, nout=0, witness=True)))
    out.append(("253 inputs", M.rand_tx(rng, 253, (25, 23))))
    out.append(("253 inputs, witness", M.rand_tx(rng, 253, (25,), witness=True)))
    out.append(("empty vin, empty vout", rng.randbytes(4) + b"\x00\x00" + rng.randbytes(4)))
    return out


@functools.lru_cache(maxsize=None)
def long_tx(seed=SEED + 1, size=40000):
    """One witness transaction of about `size` bytes (a padded witness element)."""
    rng = random.Random(seed)
    vin = [(rng.randbytes(36), rng.randbytes(20000 - 100), rng.randbytes(4))]
    return M.ser_tx(rng.randbytes(4), vin, M.rand_outs(rng, (25,)), rng.randbytes(4),
                    [[rng.randbytes(size - 20000)]])


@functools.lru_cache(maxsize=None)
def bad_tx_cases(seed=SEED + 2):
    """[(label, raw, err)]: items that do not parse or carry a trailing byte."""
    rng = random.Random(seed)
    good = M.rand_tx(rng, 2, (25, 23), witness=True)
    plain = M.rand_tx(rng, 1, (25,))
    return [("truncated", good[:-3], ERR_TX_DESERIALIZE),
            ("trailing byte", good + b"\x00", ERR_TX_SIZE_MISMATCH),
            ("trailing byte, no witness", plain + b"\x51", ERR_TX_SIZE_MISMATCH),
            ("empty", b"", ERR_TX_DESERIALIZE),
            ("superfluous witness", M.ser_tx(b"\x01\0\0\0", [(bytes(36), b"", bytes(4))], [], bytes(4),
                                            [[]]), ERR_TX_DESERIALIZE),
            ("unknown flag", plain[:4] + b"\x00\x02" + plain[4:], ERR_TX_DESERIALIZE),
            ("non-canonical count", plain[:4] + b"\xfd\x01\x00" + plain[5:], ERR_TX_DESERIALIZE)]


MERKLE_SIZES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 129, 255, 256, 257, 1000)


@functools.lru_cache(maxsize=None)
def merkle_cases(seed=SEED + 3):
    """[(label, leaves)]: random trees of every size asked for, then the mutation cases."""
    rng = random.Random(seed)
    leaf = lambda: rng.randbytes(32)
    out = [(f"n={n}", [leaf() for _ in range(n)]) for n in MERKLE_SIZES]
    a, b, c = leaf(), leaf(), leaf()
    out.append(("[a,b,c]", [a, b, c]))
    out.append(("[a,b,c,c]", [a, b, c, c]))
    p = [leaf() for _ in range(8)]
    out.append(("equal pair, second level", p[:2] + p[:2] + p[4:]))       # nodes 0 and 1 of level 1
    out.append(("equal pair, third level", p[:4] + p[:4] + [leaf() for _ in range(8)]))
    q = [leaf() for _ in range(6)]
    out.append(("equal neighbours, odd position", [q[0], q[1], q[1], q[2], q[3], q[4]]))
    out.append(("odd level's self-pair", [leaf() for _ in range(5)]))
    out.append(("odd second level", [leaf() for _ in range(6)]))
    out.append(("equal pair at the end of an even level", q[:4] + [q[5], q[5]]))
    return out


def header(root, rng):
    return rng.randbytes(36) + root + rng.randbytes(12)


def make_block(rng, txs, root=None):
    """80-byte header (with the model's root unless given) || count || txs."""
    if root is None:
        root = merkle_root([Tx(t).txid() for t in txs])[0]
    return header(root, rng) + M.cs(len(txs)) + b"".join(txs)


def coinbase(rng, outs, witness=None):
    vin = [(bytes(32) + b"\xff\xff\xff\xff", rng.randbytes(8), b"\xff\xff\xff\xff")]
    return M.ser_tx(b"\x01\0\0\0", vin, outs, bytes(4), witness)


def commit_out(commit, extra=b""):
    spk = COMMIT_HEAD + commit + extra
    return bytes(8) + M.cs(len(spk)) + spk


def segwit_block(rng, n_tx, nonce_stack="ok", commit="ok", outs_before=(), outs_after=(),
                 witness_txs=True):
    """A block of n_tx transactions whose coinbase commits to its witness tree.  nonce_stack: "ok",
    or the coinbase's witness stack; commit: "ok", "bad", None (no commitment output), or the
    scriptPubKey bytes to use."""
    rest = [M.rand_tx(rng, 1 + k % 3, (25, 22), witness=witness_txs) for k in range(n_tx - 1)]
    nonce = rng.randbytes(32)
    wroot = merkle_root([ZERO] + [Tx(t).wtxid() for t in rest])[0]
    good = sha256d(wroot + nonce)
    outs = [rng.randbytes(8) + M.cs(25) + rng.randbytes(25)] + list(outs_before)
    if commit == "ok":
        outs.append(commit_out(good))
    elif commit == "long":  # more than 38 bytes: still a commitment
        outs.append(commit_out(good, rng.randbytes(4)))
    elif commit == "bad":
        outs.append(commit_out(bytes([good[0] ^ 1]) + good[1:]))
    elif commit is not None:
        outs.append(bytes(8) + M.cs(len(commit)) + commit)
    outs += list(outs_after)
    stack = [nonce] if nonce_stack == "ok" else nonce_stack
    cb = coinbase(rng, outs, [stack] if stack is not None else None)
    return make_block(rng, [cb] + rest), good


@functools.lru_cache(maxsize=None)
def block_cases(seed=SEED + 4):
    """[(label, raw block, segwit_active)] for bcc_block_commitments_batch."""
    rng = random.Random(seed)
    out = []
    plain = lambda n: [coinbase(rng, M.rand_outs(rng, (25,)))] + [M.rand_tx(rng, 1 + k % 4, (25, 23))
                                                                 for k in range(n - 1)]
    for n in (1, 2, 3, 65, 300):
        out.append((f"{n} txs", make_block(rng, plain(n)), 1))
    out.append(("wrong header root", make_block(rng, plain(5), root=rng.randbytes(32)), 1))
    t = plain(3)
    out.append(("mutated", make_block(rng, t + [t[2]], root=merkle_root(
        [Tx(x).txid() for x in t])[0]), 1))
    out.append(("valid commitment", segwit_block(rng, 7)[0], 1))
    out.append(("valid commitment, one tx", segwit_block(rng, 1)[0], 1))
    out.append(("valid commitment, 66 txs", segwit_block(rng, 66)[0], 1))
    out.append(("reserved value of 31 bytes", segwit_block(rng, 4, [rng.randbytes(31)])[0], 1))
    out.append(("reserved value of 33 bytes", segwit_block(rng, 4, [rng.randbytes(33)])[0], 1))
    out.append(("two stack elements", segwit_block(rng, 4, [rng.randbytes(32)] * 2)[0], 1))
    out.append(("no reserved value", segwit_block(rng, 4, None)[0], 1))
    out.append(("commitment mismatch", segwit_block(rng, 5, commit="bad")[0], 1))
    out.append(("two commitments, the last wrong",
                segwit_block(rng, 5, commit="bad", outs_before=[commit_out(rng.randbytes(32))])[0], 1))
    out.append(("two commitments, the last right",
                segwit_block(rng, 5, outs_before=[commit_out(rng.randbytes(32))])[0], 1))
    out.append(("commitment with trailing script bytes", segwit_block(rng, 3, commit="long")[0], 1))
    out.append(("commitment followed by another output",
                segwit_block(rng, 3, outs_after=[M.rand_outs(rng, (25,))[0]])[0], 1))
    look = COMMIT_HEAD + rng.randbytes(31)  # 37 bytes: not a commitment
    out.append(("37-byte look-alike, no witness data",
                segwit_block(rng, 4, None, commit=look, witness_txs=False)[0], 1))
    out.append(("37-byte look-alike, witness data", segwit_block(rng, 4, commit=look)[0], 1))
    out.append(("witness tx without a commitment", segwit_block(rng, 4, None, commit=None)[0], 1))
    out.append(("segwit inactive, commitment and witness data", segwit_block(rng, 4)[0], 0))
    out.append(("segwit inactive, commitment, no witness data",
                segwit_block(rng, 4, None, witness_txs=False)[0], 0))
    whole = make_block(rng, plain(4))
    out.append(("truncated", whole[:-5], 1))
    out.append(("trailing byte", whole + b"\x00", 1))
    out.append(("short header", whole[:79], 1))
    out.append(("header only", whole[:80], 1))
    out.append(("zero count", whole[:80] + b"\x00", 1))
    out.append(("non-canonical count", whole[:80] + b"\xfd\x04\x00" + whole[81:], 1))
    out.append(("count beyond the data", whole[:80] + b"\xfd\x00\x10" + whole[81:], 1))
    return out


@functools.lru_cache(maxsize=None)
def load_fixture():
    """tests/golden/block_commit.json.gz: the header, the count and the txids of block 413567."""
    d = json.load(gzip.open(FIXTURE))
    return bytes.fromhex(d["header"]), d["transactions"], [bytes.fromhex(t) for t in d["txids"]]
