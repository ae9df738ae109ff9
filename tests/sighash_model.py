"""A plain hashlib model of the reference's three signature hashes, and the directed sweeps that
put every byte-geometry edge of the device sighash kernels (csrc/sighash.hip) under it.

The model (nothing from the code under test):
* sighash(): SignatureHash (interpreter.cpp:1576-1642) = the legacy serializer (:1273-1364) and
  BIP143 (:1366-1397, :1581-1625).  Two quirks of the legacy serializer decide whether a model
  agrees with the reference: SerializeScriptCode (:1293-1312) walks opcodes, writes compactsize
  (size - separators) and stops copying where GetOp stopped on a truncated push; SIGHASH_SINGLE
  with n_in >= vout.size() is the constant ONE (:1627-1633).
* tapsighash(): SignatureHashSchnorr (:1491-1574), BIP341 / BIP342.
test_sighash_geometry.py pins both against the committed reference goldens and, where oracle/_ref
is built, against the reference itself on every sweep check.

The sweeps (deterministic from SEED): transactions are random bytes in a chosen shape, scriptCodes
are single-byte non-push opcodes without OP_CODESEPARATOR (well-formed at every length).  Every
builder returns (checks, geometry records); a record is computed from the builder's inputs with
the formulas of pipeline.h / host/engine.cpp (TplJob, tpl_nblk, TPL_MID_MIN_BLOCKS, WinJob), never
from a value the library returns.  ECDSA-era checks are the tuples bcc_debug_sighash takes
(tx, script_code, n_in, hashtype, amount, sigversion); Taproot checks are the dicts
taproot_verify_batch takes.
"""
import functools
import hashlib
import random
import struct

SEED = 0x51D6E0
ONE = b"\x01" + bytes(31)


def sha256(b):
    return hashlib.sha256(b).digest()


def sha256d(b):
    return sha256(sha256(b))


def cs(n):
    if n < 253:
        return bytes([n])
    if n <= 0xFFFF:
        return b"\xfd" + n.to_bytes(2, "little")
    if n <= 0xFFFFFFFF:
        return b"\xfe" + n.to_bytes(4, "little")
    return b"\xff" + n.to_bytes(8, "little")


def cs_len(n):
    return 1 if n < 253 else 3 if n <= 0xFFFF else 5 if n <= 0xFFFFFFFF else 9


# ------------------------------------------------------------------------------------------------
# wire format


class _Reader:
    def __init__(self, b):
        self.b, self.i = b, 0

    def take(self, n):
        if self.i + n > len(self.b):
            raise ValueError("end of data")
        out = self.b[self.i:self.i + n]
        self.i += n
        return out

    def compact(self):
        k = self.take(1)[0]
        if k < 253:
            return k
        return int.from_bytes(self.take({253: 2, 254: 4, 255: 8}[k]), "little")


def parse_tx(raw):
    """-> dict(version, vin=[(outpoint36, scriptSig, sequence4)], vout=[serialized CTxOut],
    locktime) (4-byte fields kept as bytes); witnesses are skipped."""
    r = _Reader(bytes(raw))
    version = r.take(4)
    n = r.compact()
    witness = False
    if n == 0 and r.i < len(r.b) - 4:  # BIP144 marker, then the flag byte
        witness = r.take(1)[0] & 1 != 0
        n = r.compact()
    vin = []
    for _ in range(n):
        prev = r.take(36)
        script = r.take(r.compact())
        vin.append((prev, script, r.take(4)))
    vout = []
    for _ in range(r.compact()):
        value = r.take(8)
        ln = r.compact()
        vout.append(value + cs(ln) + r.take(ln))
    if witness:
        for _ in range(n):
            for _ in range(r.compact()):
                r.take(r.compact())
    locktime = r.take(4)
    if r.i != len(r.b):
        raise ValueError("trailing bytes")
    return dict(version=version, vin=vin, vout=vout, locktime=locktime)


def parse_outputs(raw):
    """A serialized std::vector<CTxOut> -> [(value8, script)]."""
    r = _Reader(bytes(raw))
    outs = []
    for _ in range(r.compact()):
        value = r.take(8)
        outs.append((value, r.take(r.compact())))
    if r.i != len(r.b):
        raise ValueError("trailing bytes")
    return outs


# ------------------------------------------------------------------------------------------------
# SignatureHash: legacy and BIP143

OP_PUSHDATA1, OP_PUSHDATA2, OP_PUSHDATA4, OP_CODESEPARATOR = 0x4c, 0x4d, 0x4e, 0xab


def _get_op(s, i):
    """CScript::GetOp: (ok, next position, opcode); on failure the position is where it stopped."""
    if i >= len(s):
        return False, i, None
    op = s[i]
    i += 1
    if op <= OP_PUSHDATA4:
        if op < OP_PUSHDATA1:
            n = op
        else:
            w = {OP_PUSHDATA1: 1, OP_PUSHDATA2: 2, OP_PUSHDATA4: 4}[op]
            if len(s) - i < w:
                return False, i, None
            n = int.from_bytes(s[i:i + w], "little")
            i += w
        if len(s) - i < n:
            return False, i, None
        i += n
    return True, i, op


def script_code_field(code):
    """SerializeScriptCode: compactsize(size - separators) || the script without its
    OP_CODESEPARATOR opcodes, up to where GetOp stopped."""
    code = bytes(code)
    seps, i = 0, 0
    while True:
        ok, i, op = _get_op(code, i)
        if not ok:
            break
        seps += op == OP_CODESEPARATOR
    out = bytearray(cs(len(code) - seps))
    i = begin = 0
    while True:
        ok, i, op = _get_op(code, i)
        if not ok:
            break
        if op == OP_CODESEPARATOR:
            out += code[begin:i - 1]
            begin = i
    if begin != len(code):
        out += code[begin:i]
    return bytes(out)


def legacy_preimage(t, code, n_in, hashtype):
    base, acp = hashtype & 0x1f, hashtype & 0x80
    out = bytearray(t["version"])
    inputs = [n_in] if acp else range(len(t["vin"]))
    out += cs(len(inputs))
    for k in inputs:
        prev, _, seq = t["vin"][k]
        out += prev
        out += script_code_field(code) if k == n_in else b"\x00"
        out += bytes(4) if k != n_in and base in (2, 3) else seq
    if base == 2:
        out += cs(0)
    elif base == 3:
        out += cs(n_in + 1)
        for k in range(n_in + 1):
            out += t["vout"][k] if k == n_in else b"\xff" * 8 + b"\x00"
    else:
        out += cs(len(t["vout"])) + b"".join(t["vout"])
    out += t["locktime"]
    return bytes(out) + struct.pack("<I", hashtype & 0xffffffff)


def bip143_preimage(t, code, n_in, hashtype, amount):
    base, acp = hashtype & 0x1f, hashtype & 0x80
    zero = bytes(32)
    prevouts = zero if acp else sha256d(b"".join(v[0] for v in t["vin"]))
    seqs = zero if acp or base in (2, 3) else sha256d(b"".join(v[2] for v in t["vin"]))
    if base not in (2, 3):
        outs = sha256d(b"".join(t["vout"]))
    elif base == 3 and n_in < len(t["vout"]):
        outs = sha256d(t["vout"][n_in])
    else:
        outs = zero
    prev, _, seq = t["vin"][n_in]
    code = bytes(code)
    return (t["version"] + prevouts + seqs + prev + cs(len(code)) + code +
            struct.pack("<Q", amount & 0xffffffffffffffff) + seq + outs + t["locktime"] +
            struct.pack("<I", hashtype & 0xffffffff))


def sighash(tx, script_code, n_in, hashtype, amount=0, sigversion=0):
    """SignatureHash -> the raw uint256 bytes (the ECDSA message).  sigversion 0 = BASE,
    1 = WITNESS_V0; hashtype is any 32-bit value (serialized as le32)."""
    t = parse_tx(tx)
    assert n_in < len(t["vin"])
    if sigversion == 1:
        return sha256d(bip143_preimage(t, script_code, n_in, hashtype, amount))
    if hashtype & 0x1f == 3 and n_in >= len(t["vout"]):
        return ONE
    return sha256d(legacy_preimage(t, script_code, n_in, hashtype))


# ------------------------------------------------------------------------------------------------
# SignatureHashSchnorr


def tagged(tag, msg):
    th = sha256(tag.encode())
    return sha256(th + th + msg)


def tapsighash(tx, spent, n_in, hash_type, sigversion=0, annex=None, tapleaf=bytes(32),
               codesep=0xFFFFFFFF):
    """-> the 32-byte TapSighash, or None where SignatureHashSchnorr returns false.
    sigversion 0 = TAPROOT (key path), 1 = TAPSCRIPT; annex None = absent."""
    if not (hash_type <= 3 or 0x81 <= hash_type <= 0x83):
        return None
    t = parse_tx(tx)
    so = parse_outputs(spent)
    assert len(so) == len(t["vin"]) and n_in < len(t["vin"])
    out_type = 1 if hash_type == 0 else hash_type & 3
    acp = hash_type & 0x80
    m = bytearray([0, hash_type]) + t["version"] + t["locktime"]
    if not acp:
        m += sha256(b"".join(v[0] for v in t["vin"]))
        m += sha256(b"".join(v for v, _ in so))
        m += sha256(b"".join(cs(len(s)) + s for _, s in so))
        m += sha256(b"".join(v[2] for v in t["vin"]))
    if out_type == 1:
        m += sha256(b"".join(t["vout"]))
    m.append((2 if sigversion == 1 else 0) + (annex is not None))
    if acp:
        v, s = so[n_in]
        m += t["vin"][n_in][0] + v + cs(len(s)) + s + t["vin"][n_in][2]
    else:
        m += struct.pack("<I", n_in)
    if annex is not None:
        m += sha256(cs(len(annex)) + bytes(annex))
    if out_type == 3:
        if n_in >= len(t["vout"]):
            return None
        m += sha256(t["vout"][n_in])
    if sigversion == 1:
        m += bytes(tapleaf) + b"\x00" + struct.pack("<I", codesep)
    return tagged("TapSighash", bytes(m))


# ------------------------------------------------------------------------------------------------
# sweep building blocks

# single-byte opcodes that GetOp reads as one opcode and that are not OP_CODESEPARATOR
OPCODES = bytes(list(range(0x61, 0xab)) + list(range(0xac, 0xba)))


def op_script(rng, n):
    return bytes(rng.choice(OPCODES) for _ in range(n))


def ser_tx(version, vin, vout, locktime, witness=None):
    """version / locktime: 4 bytes; vin: [(outpoint36, scriptSig, sequence4)]; vout: [serialized
    CTxOut]; witness: None or one stack (list of items) per input (BIP144 form)."""
    out = bytearray(version)
    if witness is not None:
        out += b"\x00\x01"
    out += cs(len(vin))
    for prev, script, seq in vin:
        out += prev + cs(len(script)) + script + seq
    out += cs(len(vout)) + b"".join(vout)
    if witness is not None:
        for st in witness:
            out += cs(len(st)) + b"".join(cs(len(x)) + x for x in st)
    return bytes(out + locktime)


def rand_outs(rng, script_lens):
    return [rng.randbytes(8) + cs(n) + rng.randbytes(n) for n in script_lens]


def rand_tx(rng, nin, out_script_lens=(), sig_lens=None, witness=False, wit_input=None):
    """A transaction of random bytes: nin inputs (scriptSig lengths sig_lens, default empty),
    one output per entry of out_script_lens.  witness: BIP144 form, every input with one random
    stack item, or only input wit_input when that is given (the others' stacks empty)."""
    sig_lens = sig_lens or [0] * nin
    vin = [(rng.randbytes(36), rng.randbytes(sig_lens[k]), rng.randbytes(4)) for k in range(nin)]
    wit = None
    if witness:
        wit = [[rng.randbytes(rng.randrange(1, 70))] if wit_input in (None, k) else []
               for k in range(nin)]
    return ser_tx(rng.randbytes(4), vin, rand_outs(rng, out_script_lens), rng.randbytes(4), wit)


def outs_len(out_script_lens):
    """Serialized length of the outputs without their count."""
    return sum(8 + cs_len(n) + n for n in out_script_lens)


def padded_blocks(n):
    return (n + 8) // 64 + 1


# ------------------------------------------------------------------------------------------------
# legacy SIGHASH_ALL: template jobs (K3', sha256d_tpl_lane)

TPL_MID_MIN_BLOCKS = 8


def legacy_all_type(ht):
    return ht & 0x80 == 0 and ht & 0x1f not in (2, 3)


def _random_all_type(rng):
    while True:
        ht = rng.getrandbits(32)
        if legacy_all_type(ht) and all((ht >> s) & 0xff for s in (0, 8, 16, 24)):
            return ht


def tpl_hashtypes():
    """0x01, 0x41, 0x7fffff01, 0x80000001 as a negative int32, and a random 32-bit value that
    legacy_all_type accepts (every one of its four bytes nonzero)."""
    return [0x01, 0x41, 0x7fffff01, 0x80000001 - (1 << 32), _random_all_type(random.Random(SEED))]


def tpl_geometry(nin, out_script_lens, k, code_len, ht):
    cl = code_len + cs_len(code_len)
    tpl_len = 4 + cs_len(nin) + 41 * nin + cs_len(len(out_script_lens)) + outs_len(out_script_lens) + 4
    pos = 4 + cs_len(nin) + 41 * k + 36
    L = tpl_len - 1 + cl + 4
    return dict(kind="tpl", nin=nin, k=k, pos=pos, cl=cl, code_len=code_len, tpl_len=tpl_len, L=L,
                e3=L - 4, fast=(L - 4) // 64, nblk=padded_blocks(L),
                mid=padded_blocks(tpl_len - 1 + 1 + 4) >= TPL_MID_MIN_BLOCKS,
                ht=ht & 0xffffffff)


class _Family:
    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.checks, self.geoms = [], []
        self.i = 0

    def result(self):
        return self.checks, self.geoms


def legacy_all_sweep(seed=SEED + 1):
    f = _Family(seed)
    rng = f.rng
    hts = tpl_hashtypes()

    def tx_of(nin, outs):
        return rand_tx(rng, nin, outs, witness=rng.random() < 0.2,
                       sig_lens=[rng.choice([0, 0, 3, 72]) for _ in range(nin)])

    def add(tx, nin, outs, k, code_len, ht=None):
        ht = hts[f.i % len(hts)] if ht is None else ht
        f.i += 1
        f.checks.append((tx, op_script(rng, code_len), k, ht, 0, 0))
        f.geoms.append(tpl_geometry(nin, outs, k, code_len, ht))

    code_lens = list(range(0, 141)) + list(range(253, 263))
    # the smallest messages: one input, no outputs (L = 55: one block, fast = 0; L = 56: two), and
    # the 55/56-byte edge with every hash type
    tx1 = tx_of(1, ())
    for n in range(0, 24):
        for ht in hts:
            add(tx1, 1, (), 0, n, ht)
    # from the IV: every code-field length at all four splice alignments (4 inputs, no outputs;
    # 3 inputs and two outputs)
    tx4, outs3 = tx_of(4, ()), (0, 34)
    tx3 = tx_of(3, outs3)
    for n in code_lens:
        for k in range(4):
            add(tx4, 4, (), k, n)
        add(tx3, 3, outs3, n % 3, n)
    # from the IV: every splice position a template without midstates can have (10 inputs)
    tx10 = tx_of(10, ())
    for k in range(10):
        for n in code_lens:
            add(tx10, 10, (), k, n)
    # from a midstate: 64 inputs, no outputs: every pos mod 64 (k = 63, a short code: the job
    # starts at the trailer), and every code-field length at splices in the first, a middle and
    # the last blocks
    tx64 = tx_of(64, ())
    for k in range(64):
        for n in (0, 1, 2, 3, 25, 70):
            add(tx64, 64, (), k, n)
    for n in code_lens:
        for k in (0, 1, 2, 3, 30, 31, 32, 33, 60, 61, 62, 63):
            add(tx64, 64, (), k, n)
    # a long transaction with outputs (bytes behind the last input that are not the lock time)
    outs5 = (25, 0, 34, 253, 22)
    tx40 = tx_of(40, outs5)
    for k in range(40):
        add(tx40, 40, outs5, k, (0, 25, 63, 107, 254)[k % 5])
    # the template's own count field changes width: 252 and 253 inputs (about 160 blocks a lane)
    for nin in (252, 253):
        for outs in ((), (25,)):
            tx = tx_of(nin, outs)
            for k in (0, 1, 2, 3, 126, nin - 2, nin - 1):
                for n in (0, 25, 107):
                    add(tx, nin, outs, k, n)
    return f.result()


def legacy_tx_order_sweep(seed=SEED + 2):
    """Whole transactions, input after input with one scriptCode each, as a block's inputs reach
    the kernel: consecutive lanes of a wave are consecutive inputs of one tx."""
    f = _Family(seed)
    rng = f.rng
    hts = tpl_hashtypes()
    for nin, outs, code_len in ((7, (25,), 25), (70, (), 25), (70, (34, 22), 106), (253, (), 25)):
        tx = rand_tx(rng, nin, outs)
        code = op_script(rng, code_len)
        for k in range(nin):
            ht = hts[(nin + len(outs)) % len(hts)]
            f.checks.append((tx, code, k, ht, 0, 0))
            f.geoms.append(tpl_geometry(nin, outs, k, code_len, ht))
    return f.result()


# ------------------------------------------------------------------------------------------------
# other legacy types: host preimage -> K3 (sha256d_msgs_kernel)


def legacy_other_sweep(seed=SEED + 3):
    f = _Family(seed)
    rng = f.rng
    for nin, outs in ((3, (0, 25, 70)), (5, (34, 22))):
        tx = rand_tx(rng, nin, outs, sig_lens=[rng.choice([0, 5, 107]) for _ in range(nin)])
        for code_len in list(range(0, 71)) + [252, 253, 254]:
            for ht, k in [(ht, k) for ht in (2, 3, 0x82, 0x83, 0x81)
                          for k in (range(nin) if ht & 3 == 3 else [code_len % nin])]:
                base, acp = ht & 0x1f, ht & 0x80
                cl = code_len + cs_len(code_len)
                bug = base == 3 and k >= len(outs)
                n = 4 + (1 + 36 + cl + 4 if acp else 1 + 41 * nin - 1 + cl)
                n += (1 if base == 2 else 1 + 9 * k + outs_len(outs[k:k + 1]) if base == 3
                      else 1 + outs_len(outs)) + 8
                f.checks.append((tx, op_script(rng, code_len), k, ht, 0, 0))
                f.geoms.append(dict(kind="legacy_host", nin=nin, k=k, ht=ht, code_len=code_len,
                                    single_bug=bug, pre_len=None if bug else n))
    return f.result()


# ------------------------------------------------------------------------------------------------
# BIP143 from the raw tx (K_wtx: bip143_tx_lane; K_win: bip143_in_kernel)

NIN_LIST = list(range(1, 41)) + [63, 64, 65, 113, 114, 252, 253]


def _amount(rng):
    return rng.choice([0, rng.randrange(1 << 51), rng.getrandbits(64) - (1 << 63)])


def wtx_geometry(nin, out_script_lens, sig_lens, witness, k, code_len, ht):
    """The uploaded layout (engine.cpp add_sighash_job): a BIP144 tx with outputs goes up without
    marker, flag and witnesses (add_wtx3), any other as its wire bytes."""
    stripped = witness and len(out_script_lens) > 0
    at = 4 + (2 if witness and not stripped else 0) + cs_len(nin)
    outpoints, cs3 = [], []
    for n in sig_lens:
        outpoints.append(at)
        if n >= 253:
            cs3.append(at + 36)
        at += 36 + cs_len(n) + n + 4
    cl = code_len + cs_len(code_len)
    return dict(kind="wtx", nin=nin, k=k, ht=ht, witness=witness, wtx3=stripped,
                outs_len=outs_len(out_script_lens), nout=len(out_script_lens),
                outpoint_align=sorted({o & 3 for o in outpoints}), cs3_at=cs3, cl=cl,
                code_len=code_len, pre_len=156 + cl, prevouts_len=36 * nin, seq_len=4 * nin)


def bip143_sweep(seed=SEED + 4):
    f = _Family(seed)
    rng = f.rng
    hts = (1, 2, 0x81, 0x82)

    def add(tx, nin, outs, sig_lens, witness, k, code_len, ht=None):
        ht = hts[f.i % 4] if ht is None else ht
        f.i += 1
        f.checks.append((tx, op_script(rng, code_len), k, ht, _amount(rng), 1))
        f.geoms.append(wtx_geometry(nin, outs, sig_lens, witness, k, code_len, ht))

    # every input count of the list in both wire forms; scriptSig lengths mixed so that the
    # outpoints take all alignments; output lengths walk through the residues mod 64
    j = 0
    for nin in NIN_LIST:
        for witness in (False, True):
            outs = () if j % 9 == 0 else (j % 64,) if j % 2 else (j % 23, (3 * j) % 41)
            sig_lens = [rng.choice([0, 0, 1, 2, 3, 23, 72, 107]) for _ in range(nin)]
            tx = rand_tx(rng, nin, outs, sig_lens, witness)
            for k in sorted({0, nin // 2, nin - 1}):
                add(tx, nin, outs, sig_lens, witness, k, (25, 0, 35, 71)[j % 4], 1)
                add(tx, nin, outs, sig_lens, witness, k, (27, 1, 36, 70)[j % 4])
            j += 1
    # hashOutputs: no outputs, and one and two outputs of every total length mod 64
    for witness in (False, True):
        for outs in [()] + [(n,) for n in range(64)] + [(n, 63 - n // 2) for n in range(0, 64, 3)]:
            sig_lens = [rng.choice([0, 1, 2, 3]) for _ in range(2)]
            tx = rand_tx(rng, 2, outs, sig_lens, witness)
            add(tx, 2, outs, sig_lens, witness, f.i % 2, 25, 1)
            add(tx, 2, outs, sig_lens, witness, f.i % 2, 25, 0x81)
    # the parse window: a first scriptSig of 0-140 bytes, then an input whose scriptSig length is
    # a 3-byte compact size, which so starts at every offset of the 128-byte window
    for n in range(0, 141):
        witness = n % 3 == 1
        outs = (n % 30,) if n % 5 or witness else ()
        sig_lens = [n, 253 + n % 9, 0]
        tx = rand_tx(rng, 3, outs, sig_lens, witness)
        add(tx, 3, outs, sig_lens, witness, n % 3, 25)
        add(tx, 3, outs, sig_lens, witness, (n + 1) % 3, 3)
        if n % 10 == 0:  # the same behind a BIP144 marker and flag that stay in the upload
            tx = rand_tx(rng, 3, (), sig_lens, True)
            add(tx, 3, (), sig_lens, True, 1, 25)
    # K_win preimage lengths 156 + cl over every residue mod 64, cl across the 3-byte compact size
    sig_lens = [0, 1]
    txs = [(rand_tx(rng, 2, (25, 34), sig_lens, w), w) for w in (False, True)]
    for n in list(range(0, 72)) + list(range(245, 263)):
        for ht in hts:
            for tx, w in txs:
                add(tx, 2, (25, 34), sig_lens, w, (n + w) % 2, n, ht)
    return f.result()


def bip143_single_sweep(seed=SEED + 5):
    """BIP143 SIGHASH_SINGLE: host preimage with digest slots (K1 aux messages, K2
    patch_digests_kernel, K3); the hashOutputs slot is at preimage byte len - 40."""
    f = _Family(seed)
    rng = f.rng
    outs = (25, 0)
    txs = [rand_tx(rng, 4, outs, witness=w) for w in (False, True)]
    for n in range(0, 71):
        for k in range(4):
            for ht in (3, 0x83):
                cl = n + cs_len(n)
                f.checks.append((txs[(n + k) % 2], op_script(rng, n), k, ht, _amount(rng), 1))
                f.geoms.append(dict(kind="bip143_single", nin=4, nout=2, k=k, ht=ht, code_len=n,
                                    cl=cl, pre_len=156 + cl, slot=156 + cl - 40,
                                    has_output=k < len(outs)))
    return f.result()


# ------------------------------------------------------------------------------------------------
# Taproot (KT_tx: taproot_tx_kernel; KT_msg: taproot_msg_kernel)

TAP_HASHTYPES = (0, 1, 2, 3, 0x81, 0x82, 0x83)
P2TR_LEN = 34
SPENT_LENS = list(range(0, 141)) + list(range(253, 261))


def taproot_sweep(seed=SEED + 6):
    """Checks for taproot_verify_batch with dummy signatures (64 bytes for hash_type 0, else 65).
    The reference's checker is only built for a tx that has a witness-bearing input whose spent
    output is a 34-byte OP_1 script (PrecomputedTransactionData::Init, interpreter.cpp:1436-1452),
    so one input of every tx (the last) is that; every other spent script is free."""
    f = _Family(seed)
    rng = f.rng

    def make(nin, out_lens, spent_lens, sig_lens=None):
        ready = nin - 1
        tx = rand_tx(rng, nin, out_lens, sig_lens, witness=True, wit_input=ready)
        lens = list(spent_lens)
        lens[ready] = P2TR_LEN
        scripts = [rng.randbytes(n) for n in lens]
        scripts[ready] = b"\x51\x20" + rng.randbytes(32)
        spent = cs(nin) + b"".join(rng.randbytes(8) + cs(len(s)) + s for s in scripts)
        return tx, spent, lens

    def add(t, nin, out_lens, k, ht, sv, annex=None, codesep=0xFFFFFFFF):
        tx, spent, lens = t
        assert ht & 3 != 3 or k < len(out_lens)
        f.i += 1
        f.checks.append(dict(tx=tx, spent=spent, nin=k, sig=bytes(64) + (bytes([ht]) if ht else b""),
                             pk=bytes(32), sigversion=sv, annex=annex, tapleaf=rng.randbytes(32),
                             codesep=codesep))
        f.geoms.append(dict(kind="taproot", nin=nin, k=k, ht=ht, sigversion=sv,
                            annex_len=None if annex is None else len(annex), codesep=codesep,
                            nout=len(out_lens), outs_len=outs_len(out_lens),
                            spent_len=lens[k], spent_total=sum(cs_len(n) + n for n in lens)))

    def ht_for(k, nout):
        ht = TAP_HASHTYPES[f.i % 7]
        return ht if ht & 3 != 3 or k < nout else ht - 2

    def annex_for():
        return None if f.i % 3 else b"\x50" + rng.randbytes(f.i % 37)

    # every input count of the list
    j = 0
    for nin in NIN_LIST:
        out_lens = [(7 * j + 3 * q) % 64 for q in range(j % 4)]
        t = make(nin, out_lens, [rng.choice([0, 22, 23, 34, 35, 67]) for _ in range(nin)],
                 [rng.choice([0, 0, 1, 2, 3]) for _ in range(nin)])
        for k in sorted({0, nin // 2, nin - 1}):
            for sv in (0, 1):
                add(t, nin, out_lens, k, ht_for(k, len(out_lens)), sv, annex_for(),
                    0xFFFFFFFF if f.i % 2 else f.i % 5)
        j += 1
    # spent-output script lengths: the signing input's (the ANYONECANPAY branch of KT_msg) and
    # with it sha_scriptpubkeys' message (KT_tx)
    for n in SPENT_LENS:
        out_lens = [n % 50]
        t = make(3, out_lens, [n, (n * 7) % 141, P2TR_LEN])
        for ht in (0x81, 0x82, 0x83, 0, 1):
            add(t, 3, out_lens, 0, ht, (n + ht) % 2, annex_for(), 0xFFFFFFFF if n % 2 else n % 7)
    # sha_outputs: no outputs, and every total length mod 64
    for out_lens in [[]] + [[n] for n in range(64)] + [[n, 63 - n // 2] for n in range(0, 64, 3)]:
        t = make(2, out_lens, [34, P2TR_LEN])
        for ht in (0, 1, 3, 0x81, 0x83):
            if ht & 3 != 3 or out_lens:
                add(t, 2, out_lens, 0, ht, f.i % 2, annex_for())
    # annex lengths 0-120 and none; hash type x path x annex x codesep in full on one tx
    out_lens = [25, 34]
    t = make(2, out_lens, [22, P2TR_LEN])
    for n in range(0, 121):
        for sv in (0, 1):
            add(t, 2, out_lens, f.i % 2, TAP_HASHTYPES[f.i % 7], sv, rng.randbytes(n), n % 4)
    for ht in TAP_HASHTYPES:
        for sv in (0, 1):
            for annex in (None, b"", b"\x50" + rng.randbytes(40)):
                for codesep in (0xFFFFFFFF, 0, 1, 77):
                    add(t, 2, out_lens, f.i % 2, ht, sv, annex, codesep)
    return f.result()


# ------------------------------------------------------------------------------------------------

ECDSA_FAMILIES = {
    "legacy_all": legacy_all_sweep,
    "legacy_tx_order": legacy_tx_order_sweep,
    "legacy_other": legacy_other_sweep,
    "bip143": bip143_sweep,
    "bip143_single": bip143_single_sweep,
}


@functools.lru_cache(maxsize=None)
def family(name):
    """(checks, geometry records, the model's expected digests) of one family; built once."""
    if name == "taproot":
        checks, geoms = taproot_sweep()
        exp = [tapsighash(c["tx"], c["spent"], c["nin"], c["sig"][64] if len(c["sig"]) == 65 else 0,
                          c["sigversion"], c["annex"], c["tapleaf"], c["codesep"]) for c in checks]
    else:
        checks, geoms = ECDSA_FAMILIES[name]()
        exp = [sighash(*c) for c in checks]
    assert len(checks) == len(geoms)
    return checks, geoms, exp


def mismatches(name, got, exp=None, geoms=None, limit=10):
    """The failure message of a comparison: family, index and geometry record of the first
    mismatching digests ('' when got == exp byte for byte)."""
    if exp is None:
        _, geoms, exp = family(name)
    assert len(got) == len(exp), (name, len(got), len(exp))
    bad = [i for i in range(len(exp)) if bytes(got[i]) != exp[i]]
    if not bad:
        return ""
    lines = [f"{name}: {len(bad)} of {len(exp)} digests differ from the model"]
    lines += [f"  [{i}] {geoms[i]}" for i in bad[:limit]]
    return "\n".join(lines)
