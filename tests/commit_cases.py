"""Builders and loaders for the BIP341 script-path commitment tests (bcc_taproot_commit_batch,
mi_xonly_tweak_check_tuples): plain Python integer curve arithmetic to CONSTRUCT spends and tuples,
the two routes by which the reference labels them, and the loader of
tests/golden/taproot_commit.json.gz (made by tests/golden/make_taproot_commit_fixtures.py).
No expected value ever comes from the arithmetic here: it only makes inputs."""
import ctypes
import gzip
import hashlib
import json
import os
import random

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "taproot_commit.json.gz")
# P2SH | WITNESS | TAPROOT: VerifyWitnessProgram's script path runs
FLAGS = 1 | 1 << 11 | 1 << 17
ERR_MISMATCH, ERR_CONTROL_SIZE = 39, 47


# ---- curve arithmetic (construction only) ----------------------------------------------------
def add(a, b):
    """Affine addition; None is the point at infinity."""
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return x, (lam * (a[0] - x) - a[1]) % P


def _jadd(J, b):
    """Jacobian J + affine b, b != +-J (true for the table walk below except by 2^-250 chance)."""
    if J is None:
        return b[0], b[1], 1
    X, Y, Z = J
    zz = Z * Z % P
    u2, s2 = b[0] * zz % P, b[1] * zz * Z % P
    h, r = (u2 - X) % P, (s2 - Y) % P
    if h == 0:
        raise ArithmeticError("exceptional addition")
    hh = h * h % P
    hhh, v = hh * h % P, X * hh % P
    x3 = (r * r - hhh - 2 * v) % P
    return x3, (r * (v - x3) - Y * hhh) % P, Z * h % P


_GTAB = None


def mul_g(k):
    """k G by an 8-bit fixed-base table (32 mixed additions and one inversion)."""
    global _GTAB
    if _GTAB is None:
        tab, base = [], (GX, GY)
        for _ in range(32):
            row, cur = [None], None
            for _ in range(255):
                cur = add(cur, base)
                row.append(cur)
            tab.append(row)
            base = add(cur, base)  # 256 base
        _GTAB = tab
    k %= N
    J = None
    for w in range(32):
        d = (k >> (8 * w)) & 0xFF
        if d:
            J = _jadd(J, _GTAB[w][d])
    if J is None:
        return None
    zi = pow(J[2], -1, P)
    return J[0] * zi * zi % P, J[1] * zi * zi * zi % P


def lift_x(x):
    """The even-y point with this x, or None."""
    if x >= P:
        return None
    c = (pow(x, 3, P) + 7) % P
    y = pow(c, (P + 1) // 4, P)
    if y * y % P != c:
        return None
    return x, y if y % 2 == 0 else P - y


def b32(v):
    return v.to_bytes(32, "big")


# ---- hashes ----------------------------------------------------------------------------------
def tagged(tag, msg):
    t = hashlib.sha256(tag.encode()).digest()
    return hashlib.sha256(t + t + msg).digest()


def cs(n):
    if n < 253:
        return bytes([n])
    if n <= 0xFFFF:
        return b"\xfd" + n.to_bytes(2, "little")
    return b"\xfe" + n.to_bytes(4, "little")


def seeded_script(seed, length):
    """Long scripts are stored in the golden file as (seed, length)."""
    return random.Random(seed).randbytes(length)


def tapleaf(leaf_version, script):
    return tagged("TapLeaf", bytes([leaf_version]) + cs(len(script)) + script)


def merkle_root(leaf, nodes):
    k = leaf
    for n in nodes:
        k = tagged("TapBranch", k + n if k < n else n + k)
    return k


# ---- spends ----------------------------------------------------------------------------------
def make_spend(rng, depth, script, leaf_version, nodes=None):
    """A valid script-path spend: dict(control, script, program, leaf) for a random internal key
    and a random path (or the given nodes; a node may be a callable of the running hash)."""
    p = None
    while p is None:
        px = rng.randrange(1, P)
        p = lift_x(px)
    leaf = tapleaf(leaf_version, script)
    k, path = leaf, []
    for j in range(depth):
        n = nodes[j] if nodes is not None else rng.randbytes(32)
        if callable(n):
            n = n(k)
        path.append(n)
        k = merkle_root(k, [n])
    t = int.from_bytes(tagged("TapTweak", b32(px) + k), "big")
    q = add(p, mul_g(t)) if t < N else None
    if q is None:  # t >= n or infinity: never for a hash output; keep the item well-formed
        q = (0, 0)
    control = bytes([leaf_version | (q[1] & 1)]) + b32(px) + b"".join(path)
    return dict(control=control, script=script, program=b32(q[0]), leaf=leaf)


def mutate(rng, item, what):
    """One bit of the parity / internal key / a node / the script / the program flipped."""
    c, s, q = bytearray(item["control"]), bytearray(item["script"]), bytearray(item["program"])
    if what == "parity":
        c[0] ^= 1
    elif what == "p":
        c[1 + rng.randrange(32)] ^= 1 << rng.randrange(8)
    elif what == "node":
        c[33 + rng.randrange(len(c) - 33)] ^= 1 << rng.randrange(8)
    elif what == "script":
        s[rng.randrange(len(s))] ^= 1 << rng.randrange(8)
    elif what == "q":
        q[rng.randrange(32)] ^= 1 << rng.randrange(8)
    else:
        raise ValueError(what)
    return dict(item, control=bytes(c), script=bytes(s), program=bytes(q))


def applicable_mutations(item):
    m = ["parity", "p", "q"]
    if len(item["control"]) > 33:
        m.append("node")
    if item["script"]:
        m.append("script")
    return m


def spend_tx(item):
    """A one-input tx whose witness is [script, control]."""
    wit = cs(2) + cs(len(item["script"])) + item["script"] + cs(len(item["control"])) + item["control"]
    return ((2).to_bytes(4, "little") + b"\x00\x01" + cs(1) + bytes(36) + cs(0) +
            (0xFFFFFFFF).to_bytes(4, "little") + cs(1) + (0).to_bytes(8, "little") + cs(0) + wit +
            (0).to_bytes(4, "little"))


def ref_spend(R, item):
    """(ret, serror) of the reference's VerifyScript for the spend (oracle_ctypes.Reference)."""
    ret, serr, _ = R.capture_script(b"\x51\x20" + item["program"], 0, spend_tx(item), 0, FLAGS)
    return ret, serr


def expected_commit(ret, serr):
    """The reference's whole-spend answer as bcc_taproot_commit_batch reports it."""
    assert (ret, serr) == (1, 0) or (ret == 0 and serr in (ERR_MISMATCH, ERR_CONTROL_SIZE)), (ret, serr)
    return ret, serr


class RefTweak:
    """secp256k1_xonly_pubkey_parse + secp256k1_xonly_pubkey_tweak_add_check as exported by the
    reference build."""

    def __init__(self, R):
        L = R.L
        L.secp256k1_context_create.restype = ctypes.c_void_p
        L.secp256k1_context_create.argtypes = [ctypes.c_uint]
        L.secp256k1_xonly_pubkey_parse.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p]
        L.secp256k1_xonly_pubkey_tweak_add_check.argtypes = [ctypes.c_void_p, ctypes.c_char_p,
                                                             ctypes.c_int, ctypes.c_char_p,
                                                             ctypes.c_char_p]
        self.L = L
        self.ctx = L.secp256k1_context_create(257)
        self.pk = ctypes.create_string_buffer(64)

    def check(self, q32, parity, p32, t32):
        if parity > 1:
            return 0  # the ABI's rule for a parity byte that is no parity
        if not self.L.secp256k1_xonly_pubkey_parse(self.ctx, self.pk, p32):
            return 0
        return self.L.secp256k1_xonly_pubkey_tweak_add_check(self.ctx, q32, parity, self.pk, t32)


# ---- tuples ----------------------------------------------------------------------------------
def valid_tuple(rng, t=None):
    """(q32, parity, p32, t32) with q = lift_x(p) + t G."""
    while True:
        px = rng.randrange(1, P)
        p = lift_x(px)
        if p is None:
            continue
        tv = rng.randrange(1, N) if t is None else t
        q = add(p, mul_g(tv))
        if q is not None:
            return b32(q[0]), q[1] & 1, b32(px), b32(tv)


def edge_tuples(rng):
    """[(cls, q32, parity, p32, t32)]: the rare branches no hash output reaches."""
    out = []
    q, par, p, t = valid_tuple(rng)
    out.append(("valid", q, par, p, t))
    out.append(("wrong_parity", q, par ^ 1, p, t))
    out.append(("parity_2", q, 2, p, t))
    out.append(("parity_255", q, 255, p, t))
    qv = int.from_bytes(q, "big")
    out.append(("q_plus_1", b32((qv + 1) % 2**256), par, p, t))
    out.append(("q_minus_1", b32((qv - 1) % 2**256), par, p, t))
    if qv + P < 2**256:
        out.append(("q_plus_prime", b32(qv + P), par, p, t))
    out.append(("t_zero_par0", p, 0, p, bytes(32)))
    out.append(("t_zero_par1", p, 1, p, bytes(32)))
    out.append(("t_eq_n", p, 0, p, b32(N)))
    out.append(("t_max", q, par, p, b32(2**256 - 1)))
    out.append(("t_n_plus_t", q, par, p, b32(int.from_bytes(t, "big") % (2**256 - N) + N)))
    out.append(("t_n_minus_1",) + valid_tuple(rng, N - 1))
    out.append(("t_one",) + valid_tuple(rng, 1))
    out.append(("t_two",) + valid_tuple(rng, 2))
    # t G == lift_x(p): the doubling case (d = the secret of the even-y lift)
    d = rng.randrange(1, N)
    pt = mul_g(d)
    if pt[1] & 1:
        d, pt = N - d, (pt[0], P - pt[1])
    dbl = add(pt, pt)
    out.append(("doubling", b32(dbl[0]), dbl[1] & 1, b32(pt[0]), b32(d)))
    out.append(("doubling_wrong_parity", b32(dbl[0]), (dbl[1] & 1) ^ 1, b32(pt[0]), b32(d)))
    # t G == -lift_x(p): the sum is the point at infinity
    out.append(("infinity_q0", bytes(32), 0, b32(pt[0]), b32(N - d)))
    out.append(("infinity_qp", b32(pt[0]), 0, b32(pt[0]), b32(N - d)))
    out.append(("p_off_curve", q, par, b32(5), t))
    out.append(("p_eq_prime", q, par, b32(P), t))
    out.append(("p_eq_prime_plus_1", q, par, b32(P + 1), t))
    out.append(("p_zero", q, par, bytes(32), t))
    out.append(("q_eq_prime", b32(P), 0, p, t))
    return out


def random_tuples(rng, n, valid_share=0.5):
    """[(cls, q32, parity, p32, t32)] valid rows and wrong rows (a flipped bit somewhere)."""
    out = []
    for _ in range(n):
        q, par, p, t = valid_tuple(rng)
        if rng.random() < valid_share:
            out.append(("valid", q, par, p, t))
            continue
        k = rng.randrange(4)
        if k == 0:
            par ^= 1
        else:
            rows = [None, bytearray(q), bytearray(p), bytearray(t)]
            rows[k][rng.randrange(32)] ^= 1 << rng.randrange(8)
            q, p, t = bytes(rows[1]) if k == 1 else q, bytes(rows[2]) if k == 2 else p, \
                bytes(rows[3]) if k == 3 else t
        out.append(("wrong", q, par, p, t))
    return out


def walk_tuples(rng, n, wrong_share=0.4):
    """n rows cheaply: the tweak t and the internal key both walk by random steps from a small
    table of (r, r G) pairs, so a valid row costs three affine additions and no square root; a
    share of the rows gets one flipped bit, and a few have a random x for p."""
    steps = []
    for _ in range(64):
        r = rng.randrange(1, N)
        steps.append((r, mul_g(r)))
    tv = rng.randrange(1, N)
    tg, pt = mul_g(tv), mul_g(rng.randrange(1, N))
    out = []
    while len(out) < n:
        r, rg = rng.choice(steps)
        tv, tg = (tv + r) % N, add(tg, rg)
        pt = add(pt, rng.choice(steps)[1])
        if pt is None or tg is None:
            pt = mul_g(rng.randrange(1, N))
            continue
        if rng.random() < 0.03:
            out.append(("p_random_x", rng.randbytes(32), rng.randrange(2), rng.randbytes(32), b32(tv)))
            continue
        px, p = pt[0], (pt[0], pt[1] if pt[1] % 2 == 0 else P - pt[1])
        q = add(p, tg)
        if q is None:
            continue
        row = [b32(q[0]), q[1] & 1, b32(px), b32(tv)]
        cls = "valid"
        if rng.random() < wrong_share:
            cls, k = "wrong", rng.randrange(4)
            if k == 1:
                row[1] ^= 1
            else:
                b = bytearray(row[k])
                b[rng.randrange(32)] ^= 1 << rng.randrange(8)
                row[k] = bytes(b)
        out.append((cls, *row))
    return out


def tuple_rows(ts):
    """(q, parity, p, t) concatenated rows of [(cls, q32, parity, p32, t32)]."""
    return (b"".join(t[1] for t in ts), bytes(t[2] for t in ts), b"".join(t[3] for t in ts),
            b"".join(t[4] for t in ts))


# ---- golden file -----------------------------------------------------------------------------
def load_golden():
    """(spends, tuples): spends = dicts cls, control, script, program, ret, serror, leaf (None
    where the control size is invalid); tuples = dicts cls, q, parity, p, t, verdict."""
    with gzip.open(GOLDEN, "rt") as f:
        d = json.load(f)
    spends = []
    for c in d["spends"]:
        script = (seeded_script(*c["script_seed"]) if "script_seed" in c
                  else bytes.fromhex(c["script"]))
        for off, bit in c.get("script_flip", []):
            b = bytearray(script)
            b[off] ^= bit
            script = bytes(b)
        control = (seeded_script(*c["control_seed"]) if "control_seed" in c
                   else bytes.fromhex(c["control"]))
        spends.append(dict(cls=c["cls"], control=control, script=script,
                           program=bytes.fromhex(c["program"]), ret=c["ret"], serror=c["serror"],
                           leaf=None if c["leaf"] is None else bytes.fromhex(c["leaf"])))
    tuples = [dict(cls=c["cls"], q=bytes.fromhex(c["q"]), parity=c["parity"],
                   p=bytes.fromhex(c["p"]), t=bytes.fromhex(c["t"]), verdict=c["verdict"])
              for c in d["tuples"]]
    return spends, tuples
