"""A plain-Python model of what the rule entries compute (include/bcc_amd.h bcc_tx_check_batch,
bcc_block_check_batch), over bytes and integers only.

It restates, independently of the engine: UnserializeTransaction with its zero-input / segwit
marker ambiguity (primitives/transaction.h:188-224), CheckTransaction
(consensus/tx_check.cpp:10-58), CScript::GetSigOpCount(false) with GetScriptOp's push rules
(script/script.cpp:152-176, 281-331), GetLegacySigOpCount and IsFinalTx
(consensus/tx_verify.cpp:17-28, 107-119), CScript() << n (script.h push_int64,
CScriptNum::serialize) and the order of CheckBlock / ContextualCheckBlock
(validation.cpp:3387-3416, 3543-3620).  The commitment fields and statuses are block_model.py's.
"""
import block_model as BM

TX_OK = 0
VIN_EMPTY, VOUT_EMPTY, OVERSIZE, VOUT_NEGATIVE, VOUT_TOOLARGE, TXOUTTOTAL_TOOLARGE = 16, 17, 18, 19, 20, 21
INPUTS_DUPLICATE, CB_LENGTH, PREVOUT_NULL = 22, 23, 24
ERR_TX_SIZE_MISMATCH, ERR_TX_DESERIALIZE = 2, 3
ERR_LENGTH, ERR_CB_MISSING, ERR_CB_MULTIPLE, ERR_TX, ERR_SIGOPS, ERR_NONFINAL, ERR_CB_HEIGHT, ERR_WEIGHT = \
    8, 9, 10, 11, 12, 13, 14, 15
SEGWIT_ACTIVE, BIP34_ACTIVE = 1, 2
MAX_MONEY = 21000000 * 100000000
MAX_WEIGHT = 4000000
MAX_SIGOPS_COST = 80000
LOCKTIME_THRESHOLD = 500000000
NULL_PREVOUT = bytes(32) + b"\xff" * 4


class End(ValueError):
    pass


def _take(b, i, n):
    if i + n > len(b):
        raise End("end of data")
    return b[i:i + n], i + n


def _compact(b, i):
    """ReadCompactSize with the canonical and MAX_SIZE checks (serialize.h:318-347)."""
    k, i = _take(b, i, 1)
    k = k[0]
    if k < 253:
        return k, i
    v, i = _take(b, i, {253: 2, 254: 4, 255: 8}[k])
    v = int.from_bytes(v, "little")
    if v < {253: 253, 254: 0x10000, 255: 1 << 32}[k] or v > 0x02000000:
        raise End("non-canonical or oversized CompactSize")
    return v, i


def _vin(b, i):
    n, i = _compact(b, i)
    vin = []
    for _ in range(n):
        prev, i = _take(b, i, 36)
        m, i = _compact(b, i)
        script, i = _take(b, i, m)
        seq, i = _take(b, i, 4)
        vin.append((prev, script, int.from_bytes(seq, "little")))
    return vin, i


def _vout(b, i):
    n, i = _compact(b, i)
    vout = []
    for _ in range(n):
        v, i = _take(b, i, 8)
        m, i = _compact(b, i)
        script, i = _take(b, i, m)
        vout.append((int.from_bytes(v, "little", signed=True), script))
    return vout, i


def parse(b, i=0):
    """UnserializeTransaction with fAllowWitness: dict(vin, vout, witness, lock_time, end,
    stripped_size); raises End where the reference throws."""
    start = i
    _, i = _take(b, i, 4)
    vin, i = _vin(b, i)
    vout, witness, flags = [], None, 0
    body0 = start + 4
    if not vin:
        f, i = _take(b, i, 1)
        flags = f[0]
        if flags != 0:
            body0 = i
            vin, i = _vin(b, i)
            vout, i = _vout(b, i)
    else:
        vout, i = _vout(b, i)
    body1 = i
    if flags & 1:
        flags ^= 1
        witness = []
        for _ in vin:
            n, i = _compact(b, i)
            st = []
            for _ in range(n):
                m, i = _compact(b, i)
                x, i = _take(b, i, m)
                st.append(x)
            witness.append(st)
        if not any(witness):
            raise End("superfluous witness record")
    if flags:
        raise End("unknown optional data")
    lt, i = _take(b, i, 4)
    stripped = 4 + (body1 - body0) + 4 if witness is not None else i - start
    return dict(vin=vin, vout=vout, witness=witness, lock_time=int.from_bytes(lt, "little"), end=i,
                stripped_size=stripped, total_size=i - start)


def script_sigops(s):
    """CScript::GetSigOpCount(false)."""
    n, i = 0, 0
    while i < len(s):
        op = s[i]
        i += 1
        if op <= 0x4e:
            size = op
            if op >= 0x4c:
                w = {0x4c: 1, 0x4d: 2, 0x4e: 4}[op]
                if len(s) - i < w:
                    break
                size = int.from_bytes(s[i:i + w], "little")
                i += w
            if len(s) - i < size:
                break
            i += size
        elif op in (0xac, 0xad):
            n += 1
        elif op in (0xae, 0xaf):
            n += 20
    return n


def legacy_sigops(t):
    return sum(script_sigops(s) for _, s, _ in t["vin"]) + sum(script_sigops(s) for _, s in t["vout"])


def is_coinbase(t):
    return len(t["vin"]) == 1 and t["vin"][0][0] == NULL_PREVOUT


def check_transaction(t):
    if not t["vin"]:
        return VIN_EMPTY
    if not t["vout"]:
        return VOUT_EMPTY
    if t["stripped_size"] * 4 > MAX_WEIGHT:
        return OVERSIZE
    total = 0
    for v, _ in t["vout"]:
        if v < 0:
            return VOUT_NEGATIVE
        if v > MAX_MONEY:
            return VOUT_TOOLARGE
        total += v
        if total > MAX_MONEY:
            return TXOUTTOTAL_TOOLARGE
    if len({p for p, _, _ in t["vin"]}) != len(t["vin"]):
        return INPUTS_DUPLICATE
    if is_coinbase(t):
        if not 2 <= len(t["vin"][0][1]) <= 100:
            return CB_LENGTH
    elif any(p == NULL_PREVOUT for p, _, _ in t["vin"]):
        return PREVOUT_NULL
    return TX_OK


def is_final(t, height, cutoff):
    lt = t["lock_time"]
    if lt == 0:
        return True
    if lt < (height if lt < LOCKTIME_THRESHOLD else cutoff):
        return True
    return all(seq == 0xffffffff for _, _, seq in t["vin"])


def push_int(n):
    """The bytes of CScript() << n."""
    if n == -1 or 1 <= n <= 16:
        return bytes([n + 0x50])
    if n == 0:
        return b"\x00"
    neg, a, out = n < 0, abs(n), bytearray()
    while a:
        out.append(a & 0xff)
        a >>= 8
    if out[-1] & 0x80:
        out.append(0x80 if neg else 0)
    elif neg:
        out[-1] |= 0x80
    return bytes([len(out)]) + bytes(out)


ZERO_TX = dict(n_in=0, n_out=0, sigops=0, lock_time=0, stripped_size=0, total_size=0, is_coinbase=0,
               all_final=0)


def tx_result(raw):
    """The bcc_tx_check_result of one item."""
    raw = bytes(raw)
    try:
        t = parse(raw)
    except End:
        return dict(ZERO_TX, status=ERR_TX_DESERIALIZE)
    if t["end"] != len(raw):
        return dict(ZERO_TX, status=ERR_TX_SIZE_MISMATCH)
    return dict(status=check_transaction(t), n_in=len(t["vin"]), n_out=len(t["vout"]),
                sigops=legacy_sigops(t), lock_time=t["lock_time"], stripped_size=t["stripped_size"],
                total_size=len(raw), is_coinbase=int(is_coinbase(t)),
                all_final=int(all(s == 0xffffffff for _, _, s in t["vin"])))


def block_result(raw, height, cutoff, flags):
    """The bcc_block_check_result of one block."""
    raw = bytes(raw)
    c = BM.block_result(raw, 1 if flags & SEGWIT_ACTIVE else 0)
    out = dict(status=c["status"], tx_index=-1, tx_status=0, n_tx=c["n_tx"], commit_pos=c["commit_pos"],
               sigops=0, stripped_size=0, weight=0, merkle_root=c["merkle_root"],
               witness_root=c["witness_root"])
    if c["status"] in (BM.ERR_DESERIALIZE, BM.ERR_EMPTY):
        return out
    n, i = _compact(raw, 80)
    txs = []
    for _ in range(n):
        t = parse(raw, i)
        i = t["end"]
        txs.append(t)
    out["sigops"] = sum(legacy_sigops(t) for t in txs)
    out["stripped_size"] = 80 + (i - 80 - sum(t["total_size"] for t in txs)) + sum(t["stripped_size"] for t in txs)
    out["weight"] = 3 * out["stripped_size"] + len(raw)
    if c["status"] in (BM.ERR_MERKLE_ROOT, BM.ERR_DUPLICATE):
        return out

    def first(pred):
        return next((k for k, t in enumerate(txs) if pred(t)), None)

    bad = first(lambda t: check_transaction(t) != TX_OK)
    nonfinal = first(lambda t: not is_final(t, height, cutoff))
    want = push_int(height)
    if n * 4 > MAX_WEIGHT or out["stripped_size"] * 4 > MAX_WEIGHT:
        out["status"] = ERR_LENGTH
    elif not is_coinbase(txs[0]):
        out["status"] = ERR_CB_MISSING
    elif any(is_coinbase(t) for t in txs[1:]):
        out["status"] = ERR_CB_MULTIPLE
    elif bad is not None:
        out.update(status=ERR_TX, tx_index=bad, tx_status=check_transaction(txs[bad]))
    elif out["sigops"] * 4 > MAX_SIGOPS_COST:
        out["status"] = ERR_SIGOPS
    elif nonfinal is not None:
        out.update(status=ERR_NONFINAL, tx_index=nonfinal)
    elif flags & BIP34_ACTIVE and txs[0]["vin"][0][1][:len(want)] != want:
        out["status"] = ERR_CB_HEIGHT
    elif c["status"]:
        out["status"] = c["status"]
    elif out["weight"] > MAX_WEIGHT:
        out["status"] = ERR_WEIGHT
    return out
