"""Generate tests/golden/structured_scalars.npz (run where the reference build oracle/_ref exists):

    python3 tests/golden/make_structured_scalars.py

Signature rows built from CHOSEN ladder scalars, for every kernel that runs a ladder.  An ECDSA row
starts from (Q, u1, u2): R = u1 G + u2 Q, r = x(R) mod n, s = r / u2, m = u1 s, so the verifier's
u1 = m / s and u2 = r / s are exactly the chosen values (the way make_fixtures.py builds its
`structured_valid` class).  Every row has an invalid twin (m + 1 or r + 1).

  u1 (the 16-bit comb)   2^k, 2^k +- 1, n - 2^k for k = 0..255 and their negations (odd and even);
                         every window of the recoded scalar at each pattern that selects table
                         index 0 or 32767 with either sign (and the plain all-zeros / all-ones
                         windows), the rest random, as u1 itself and as n - u1; 0
  u2 (GLV, 4-bit digits) a + lambda b over a signed edge set (0, +-1, +-2, +-15, +-16, +-17,
                         +-2^64, +-2^124, +-(2^125 + 1), +-(2^126 - 1)): lambda, -lambda,
                         lambda +- 1, a half equal to zero, every sign / parity combination
  both                   residues below NC = 2^256 - n and in [NC, 2 NC): the products r s^-1 and
                         m s^-1 then take the last steps of the mod-n reduction (scalar_cases.py)
  keys                   the structured keys of make_fixtures.py plus random ones; compressed,
                         uncompressed and hybrid encodings

The same u1 families as tweak rows (q, parity, p, t) with t the comb scalar, and BIP340 rows: valid
ones from structured keys and nonces, and rows with a structured s.  (A valid BIP340 signature with
a chosen s or challenge cannot be built: the challenge hashes R and the key.  Rows with a chosen s
therefore carry a foreign R and are invalid; they still run the whole ladder.)

Every verdict comes from the REFERENCE (CPubKey::Verify, secp256k1_schnorrsig_verify,
secp256k1_xonly_pubkey_tweak_add_check); a plain Python integer model of each check is asserted to
agree with it.  The coverage conditions are asserted on the Python model of the split and the
recodings (scalar_cases.py) and recorded in the file's header."""
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import commit_cases as C  # noqa: E402
import scalar_cases as S  # noqa: E402
from make_fixtures import der, tagged_hash  # noqa: E402
from oracle_ctypes import Reference  # noqa: E402

P, N, NC, LAM, M = S.P, S.N, S.NC, S.LAM, S.M
OUT = os.path.join(HERE, "structured_scalars.npz")
WC, CWIN, CTAB = 16, 16, 32768
WQ, QWIN, QTAB = 4, 32, 8


def inv(a):
    return pow(a, -1, N)


def mul(k):
    """k G (None: infinity)."""
    return C.mul_g(k % N)


# ---- models of what the lanes do with u1 / u2 (coverage only) ----------------------------------
def comb_indices(u1):
    """[(index, negative)] per window of the comb over the odd form of u1 (n - u1 when even)."""
    u = u1 if u1 & 1 else N - u1
    return [((abs(d) - 1) // 2, d < 0) for d in S.recode_model(u, WC, CWIN)]


def q_model(u2):
    """(flags NEG0 NEG1 CORR0 CORR1, zero halves, [(idx, neg)] of slot 0, of slot 1)."""
    k1, k2 = (S.signed(v) for v in S.split_model(u2))
    assert abs(k1) < 2**128 and abs(k2) < 2**128
    flags = (k1 < 0, k2 < 0, abs(k1) % 2 == 0, abs(k2) % 2 == 0)
    digs = [[((abs(d) - 1) // 2, d < 0) for d in S.recode_model(abs(k) | 1, WQ, QWIN)]
            for k in (k1, k2)]
    return flags, (k1 == 0, k2 == 0), digs[0], digs[1]


# ---- scalar families ---------------------------------------------------------------------------
def u1_family(rng):
    out = [("u1_zero", 0)]
    for k in range(256):
        for name, v in (("pow2", 2**k), ("pow2_plus", 2**k + 1), ("pow2_minus", 2**k - 1),
                        ("n_minus_pow2", N - 2**k)):
            out.append(("u1_" + name, v % N))
            out.append(("u1_" + name + "_neg", -v % N))
    # the digit of window i reads bits 16 i + 1 .. 16 i + 16 of the odd scalar: 0x0000 -> (32767, -),
    # 0xFFFF -> (32767, +), 0x8000 -> (0, +), 0x7FFF -> (0, -); the top digit is the plain 15 bits
    for win in range(CWIN):
        for pat in (0x0000, 0xFFFF, 0x8000, 0x7FFF):
            for _ in range(2):
                v = rng.randrange(N) | 1
                mask = 0xFFFF << (WC * win + 1)
                v = (v & ~mask | pat << (WC * win + 1)) & (M - 1)
                if win == CWIN - 1:  # the top digit's 15 bits; keep the value below n
                    v = v & ~(0xFFFF << 241) | (0x7FFF if pat in (0xFFFF, 0x7FFF) else 0) << 241
                    if v >= N:
                        v -= 2**200
                assert v & 1 and 0 < v < N
                out.append(("u1_window", v))
                out.append(("u1_window_even", N - v))
        for pat in (0x0000, 0xFFFF):  # the plain windows, both parities
            for low in (0, 1):
                v = rng.randrange(N)
                v = (v & ~(0xFFFF << (WC * win)) | pat << (WC * win)) & ~1 | low
                if 0 < v < N:
                    out.append(("u1_plain_window", v))
    return out


U2_EDGE = [0, 1, -1, 2, -2, 15, -15, 16, -16, 17, -17, 2**64, -(2**64), 2**124, -(2**124),
           2**125 + 1, -(2**125 + 1), 2**126 - 1, -(2**126 - 1)]


def u2_family():
    out = []
    for a in U2_EDGE:
        for b in U2_EDGE:
            if a or b:
                k = (a + LAM * b) % N
                assert tuple(S.signed(v) for v in S.split_model(k)) == (a, b)
                out.append(("u2_glv", k))
    assert {LAM, N - LAM, LAM + 1, LAM - 1} <= {k for _, k in out}
    return out


# ---- ECDSA -------------------------------------------------------------------------------------
def py_ecdsa(q, m, r, s):
    """ECDSA over the key q G on integers: x(u1 G + u2 Q) mod n == r."""
    if not (0 < r < N and 0 < s < N):
        return 0
    si = inv(s)
    Rp = mul(m % N * si + r * si * q)
    return int(Rp is not None and Rp[0] % N == r)


def ecdsa_row(q, u1, u2):
    """(r, s, m) with m / s == u1 and r / s == u2, or None when R is infinity or r == 0."""
    Rp = mul(u1 + u2 * q)
    if Rp is None or Rp[0] % N == 0 or u2 % N == 0:
        return None
    r = Rp[0] % N
    s = r * inv(u2) % N
    return r, s, u1 * s % N


def make_ecdsa(R, rng):
    secrets = [1, 2, 3, N - 1, N - 2, LAM, LAM * LAM % N, 2**128, 2**128 + 1, 2**127, 7]
    secrets += [rng.randrange(1, N) for _ in range(21)]
    points = [mul(q) for q in secrets]
    u1s, u2s = u1_family(rng), u2_family()
    plan = []  # (cls, key, u1, u2)
    for i, (cls, u1) in enumerate(u1s):
        plan.append((cls, i % len(secrets), u1, u2s[i % len(u2s)][1]))
    for i, (cls, u2) in enumerate(u2s):  # every u2 again with a random u1 and the next key
        plan.append((cls, (7 * i + 3) % len(secrets), rng.randrange(1, N), u2))
    for i in range(len(secrets)):  # lambda and its neighbours on every key
        for u2 in (LAM, N - LAM, LAM + 1, LAM - 1):
            plan.append(("u2_lambda", i, rng.randrange(1, N), u2))
    for i, q in enumerate(secrets):  # u1 G == +-u2 Q: the final sum doubles or vanishes (R infinity)
        for j in range(6):
            u2 = u2s[(53 * i + 17 * j) % len(u2s)][1] if j < 4 else rng.randrange(1, N)
            plan.append(("a_equals_b", i, u2 * q % N, u2))
            plan.append(("a_equals_minus_b", i, -u2 * q % N, u2))
    for i in range(150):  # random scalars: the digits no family pins (the top Q digits among them)
        plan.append(("random", i % len(secrets), rng.randrange(1, N), rng.randrange(1, N)))
    rows, skipped = [], 0
    for cls, ki, u1, u2 in plan:
        got = ecdsa_row(secrets[ki], u1, u2)
        if got is None:  # R at infinity: the row as make_fixtures' `structured` class (s = 1)
            skipped += 1
            if u2 % N:
                rows.append((cls + "_s1", ki, u2 % N, 1, u1 % N, u1, u2))
            continue
        rows.append((cls, ki, *got, u1, u2))
    # residues that drive the reduction's last steps: keep drawing until enough products carry
    carry = ge_n = 0
    while carry < 60 or ge_n < 300:
        lo, hi = ((0, NC) if ge_n < 300 and rng.random() < 0.5 else (NC, 2 * NC))
        ki = rng.randrange(len(secrets))
        u1, u2 = rng.randrange(max(lo, 1), hi), rng.randrange(max(lo, 1), hi)
        got = ecdsa_row(secrets[ki], u1, u2)
        if got is None:
            continue
        r, s, m = got
        cov = S.mul_coverage([(r, inv(s)), (m, inv(s))])
        if lo == 0 and ge_n < 300:
            assert cov["ge_n"] == 2
            ge_n += 1
            rows.append(("reduce_below_nc", ki, r, s, m, u1, u2))
        elif cov["carry"]:
            carry += 1
            rows.append(("reduce_carry", ki, r, s, m, u1, u2))
    rng.shuffle(rows)

    n = len(rows)
    keys = np.zeros((len(points), 64), np.uint8)
    for i, pt in enumerate(points):
        keys[i] = np.frombuffer(C.b32(pt[0]) + C.b32(pt[1]), np.uint8)
    out = dict(e_keys=keys, e_key=np.zeros(n, np.uint8), e_kind=np.zeros(n, np.uint8),
               e_hash=np.zeros((n, 32), np.uint8), e_r=np.zeros((n, 32), np.uint8),
               e_s=np.zeros((n, 32), np.uint8), e_twin=np.zeros(n, np.uint8),
               e_verdict=np.zeros(n, np.uint8), e_twin_verdict=np.zeros(n, np.uint8),
               e_cls=np.zeros(n, np.uint8))
    classes = sorted({r[0] for r in rows})
    cover = dict(flags=set(), zero_half=set(), qidx=[set(), set()], qtop=[set(), set()],
                 comb=[set() for _ in range(CWIN)], comb_sign=[set() for _ in range(CWIN)],
                 fold_carry_rows=0, fold_ge_n_rows=0, u1_zero=0)
    for i, (cls, ki, r, s, m, u1, u2) in enumerate(rows):
        kind = i % 3
        pub = ecdsa_pub(points[ki], kind)
        twin = 1 + (i & 1)
        tm, tr = ((m + 1) % M, r) if twin == 1 else (m, r + 1)
        v = R.pubkey_verify(pub, C.b32(m), der(r, s))
        tv = R.pubkey_verify(pub, C.b32(tm), der(tr, s))
        assert v == py_ecdsa(secrets[ki], m, r, s), (cls, i)
        assert tv == py_ecdsa(secrets[ki], tm, tr, s), (cls, i)
        assert v == 1 or cls.endswith("_s1")
        out["e_key"][i], out["e_kind"][i], out["e_twin"][i] = ki, kind, twin
        out["e_hash"][i] = np.frombuffer(C.b32(m), np.uint8)
        out["e_r"][i] = np.frombuffer(C.b32(r), np.uint8)
        out["e_s"][i] = np.frombuffer(C.b32(s), np.uint8)
        out["e_verdict"][i], out["e_twin_verdict"][i] = v, tv
        out["e_cls"][i] = classes.index(cls)
        # coverage of what the lanes derive: u1 = m / s, u2 = r / s
        si = inv(s)
        assert (m * si % N, r * si % N) == (u1 % N, u2 % N)
        flags, zero, d0, d1 = q_model(u2 % N)
        cover["flags"].add(flags)
        cover["zero_half"] |= {j for j in (0, 1) if zero[j]}
        for slot, ds in enumerate((d0, d1)):
            cover["qidx"][slot] |= {ix for ix, _ in ds[:-1]}
            cover["qtop"][slot].add(ds[-1][0])
        if u1 % N == 0:
            cover["u1_zero"] += 1
        else:
            for w, (ix, ng) in enumerate(comb_indices(u1 % N)):
                cover["comb"][w].add(ix)
                if ix in (0, CTAB - 1):
                    cover["comb_sign"][w].add((ix, ng))
        cov = S.mul_coverage([(r, si), (m, si)])
        cover["fold_carry_rows"] += cov["carry"] > 0
        cover["fold_ge_n_rows"] += cov["ge_n"] > 0
    assert len(cover["flags"]) == 16, sorted(cover["flags"])
    assert cover["zero_half"] == {0, 1}
    assert all(s == set(range(QTAB)) for s in cover["qidx"])
    assert all({0, CTAB - 1} <= s for s in cover["comb"])
    assert all(len(s) == 4 for s in cover["comb_sign"][:-1]) and len(cover["comb_sign"][-1]) == 2
    assert cover["fold_carry_rows"] >= 30 and cover["u1_zero"] >= 1
    header = dict(ecdsa_rows=n, ecdsa_valid=int(out["e_verdict"].sum()),
                  ecdsa_twin_valid=int(out["e_twin_verdict"].sum()), r_infinity_plans=skipped,
                  flag_combinations=len(cover["flags"]), zero_halves=sorted(cover["zero_half"]),
                  q_indices=[sorted(s) for s in cover["qidx"]],
                  q_top_indices=[sorted(s) for s in cover["qtop"]],
                  comb_extremes_every_window=True,
                  comb_distinct_indices=[len(s) for s in cover["comb"]],
                  fold_carry_rows=int(cover["fold_carry_rows"]),
                  fold_ge_n_rows=int(cover["fold_ge_n_rows"]), u1_zero_rows=cover["u1_zero"])
    return out, classes, header


def ecdsa_pub(pt, kind):
    x, y = C.b32(pt[0]), C.b32(pt[1])
    if kind == 0:
        return bytes([2 + (pt[1] & 1)]) + x
    return bytes([4 if kind == 1 else 6 + (pt[1] & 1)]) + x + y


# ---- tweak rows --------------------------------------------------------------------------------
def make_tweak(R, rng):
    RT = C.RefTweak(R)
    ds = []
    while len(ds) < 16:  # internal keys: the even-y lifts of d G
        d = rng.randrange(1, N)
        ds.append(d if mul(d)[1] % 2 == 0 else N - d)
    ds[0] = 1 if mul(1)[1] % 2 == 0 else N - 1
    pts = [mul(d) for d in ds]
    rows = []
    for i, (cls, t) in enumerate(u1_family(rng)):
        ki = i % len(ds)
        q = mul(ds[ki] + t)
        if q is None:
            continue
        par = q[1] & 1
        twin = 1 + (i & 1)  # 1: the other parity, 2: x(q) + 1
        rows.append((cls.replace("u1_", "t_"), ki, q[0], par, t, twin))
    rng.shuffle(rows)
    n = len(rows)
    keys = np.zeros((len(pts), 32), np.uint8)
    for i, pt in enumerate(pts):
        keys[i] = np.frombuffer(C.b32(pt[0]), np.uint8)
    classes = sorted({r[0] for r in rows})
    out = dict(t_keys=keys, t_key=np.zeros(n, np.uint8), t_q=np.zeros((n, 32), np.uint8),
               t_parity=np.zeros(n, np.uint8), t_t=np.zeros((n, 32), np.uint8),
               t_twin=np.zeros(n, np.uint8), t_verdict=np.zeros(n, np.uint8),
               t_twin_verdict=np.zeros(n, np.uint8), t_cls=np.zeros(n, np.uint8))
    comb = [set() for _ in range(CWIN)]
    for i, (cls, ki, qx, par, t, twin) in enumerate(rows):
        p32, t32 = C.b32(pts[ki][0]), C.b32(t)
        tq, tpar = (qx, par ^ 1) if twin == 1 else ((qx + 1) % M, par)
        v = RT.check(C.b32(qx), par, p32, t32)
        tv = RT.check(C.b32(tq), tpar, p32, t32)
        assert v == 1 and tv == 0, (cls, i, v, tv)  # the integer model: q = lift_x(p) + t G exactly
        out["t_key"][i], out["t_parity"][i], out["t_twin"][i] = ki, par, twin
        out["t_q"][i] = np.frombuffer(C.b32(qx), np.uint8)
        out["t_t"][i] = np.frombuffer(t32, np.uint8)
        out["t_verdict"][i], out["t_twin_verdict"][i] = v, tv
        out["t_cls"][i] = classes.index(cls)
        if t:
            for w, (ix, _) in enumerate(comb_indices(t)):
                comb[w].add(ix)
    assert all({0, CTAB - 1} <= s for s in comb)
    return out, classes, dict(tweak_rows=n)


# ---- BIP340 ------------------------------------------------------------------------------------
def py_schnorr(d_even, px, sig, msg):
    rx, s = int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")
    if rx >= P or s >= N:
        return 0
    e = int.from_bytes(tagged_hash(b"BIP0340/challenge", sig[:32] + C.b32(px) + msg), "big") % N
    Rp = mul(s - e * d_even)
    return int(Rp is not None and Rp[1] % 2 == 0 and Rp[0] == rx)


def make_schnorr(R, rng):
    rows = []  # (cls, d_even, px, sig, msg)

    def sign(d, k, msg):
        pt = mul(d)
        de = d if pt[1] % 2 == 0 else N - d
        Rp = mul(k)
        if Rp[1] & 1:
            k = N - k
        e = int.from_bytes(tagged_hash(b"BIP0340/challenge", C.b32(Rp[0]) + C.b32(pt[0]) + msg),
                           "big") % N
        return de, pt[0], C.b32(Rp[0]) + C.b32((k + e * de) % N)

    keys = [1, 2, 3, 7, N - 1, N - 2, LAM, N - LAM, LAM + 1, 2**128, 2**127 + 1, 2**255]
    nonces = [1, 2, 3, N - 1, LAM, N - LAM, 2**64, 2**128 - 1, 2**128, 2**255, (N + 1) // 2]
    for d in keys + [rng.randrange(1, N) for _ in range(8)]:
        for k in nonces + [rng.randrange(1, N) for _ in range(3)]:
            msg = rng.choice([bytes(32), b"\xff" * 32, rng.randbytes(32)])
            de, px, sig = sign(d, k, msg)
            rows.append(("valid_structured_key_nonce", de, px, sig, msg))
            bad = bytearray(sig)
            bad[32 + rng.randrange(32)] ^= 1 << rng.randrange(8)
            rows.append(("structured_key_nonce_s_flip", de, px, bytes(bad), msg))
    # a chosen s (the comb's scalar) under a foreign R: the u1 families, thinned
    fam = u1_family(rng)
    picks = [f for f in fam if "window" in f[0]] + fam[1:1 + 8 * 64:8] + [fam[0]]
    for i, (cls, sv) in enumerate(picks):
        d = rng.randrange(1, N)
        msg = rng.randbytes(32)
        de, px, sig = sign(d, rng.randrange(1, N), msg)
        rows.append((cls.replace("u1_", "s_"), de, px, sig[:32] + C.b32(sv), msg))
    rng.shuffle(rows)
    n = len(rows)
    classes = sorted({r[0] for r in rows})
    out = dict(s_sig=np.zeros((n, 64), np.uint8), s_msg=np.zeros((n, 32), np.uint8),
               s_pub=np.zeros((n, 32), np.uint8), s_verdict=np.zeros(n, np.uint8),
               s_cls=np.zeros(n, np.uint8))
    for i, (cls, de, px, sig, msg) in enumerate(rows):
        v = R.schnorr_verify(sig, msg, C.b32(px))
        assert v == py_schnorr(de, px, sig, msg), (cls, i)
        out["s_sig"][i] = np.frombuffer(sig, np.uint8)
        out["s_msg"][i] = np.frombuffer(msg, np.uint8)
        out["s_pub"][i] = np.frombuffer(C.b32(px), np.uint8)
        out["s_verdict"][i] = v
        out["s_cls"][i] = classes.index(cls)
    return out, classes, dict(schnorr_rows=n, schnorr_valid=int(out["s_verdict"].sum()))


def main():
    R = Reference()
    rng = random.Random(0x5EED5CA1)
    e, ecls, eh = make_ecdsa(R, rng)
    t, tcls, th = make_tweak(R, rng)
    s, scls, sh = make_schnorr(R, rng)
    header = dict(eh, **th, **sh)
    np.savez_compressed(OUT, **e, **t, **s, e_classes=np.array(ecls), t_classes=np.array(tcls),
                        s_classes=np.array(scls), header=np.array(json.dumps(header)))
    print(json.dumps(header))
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
