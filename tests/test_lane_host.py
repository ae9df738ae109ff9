"""CPU: the kernel's per-lane arithmetic (csrc/ecdsa_lane.h, compiled for the host by
tests/native/lane_host.cpp -- test-only, never part of the product) against the reference
fixtures. Lets the exact lane code be checked without a GPU."""
import ctypes
import os
import random
import subprocess

import pytest

from fixtures import bip340_vectors, ecdsa_tuples, pub_to_tuple, schnorr_tuples
from oracle_ctypes import Oracle, Reference, reference_available

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "native", "_build", "lane_host.so")


def _build_lane(so, extra=()):
    src = os.path.join(HERE, "native", "lane_host.cpp")
    deps = [src] + [os.path.join(HERE, "..", "rust-bitcoinconsensus_amd", "csrc", f)
                    for f in ("ecdsa_lane.h", "ecdsa_twist.h", "secp256k1_device.h", "modinv_host.h",
                              "modinv_device.h", "sha256_device.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", *extra, "-o", so, src])
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def lane():
    return _build_lane(SO)


# The host builds of the arithmetic: 4 x 64-bit limbs with 128-bit products (BCC_FE_HOST64, what the
# host engine runs) and, without __int128, the portable 8 x 32-bit formulation -- the same
# sc_reduce512 column folds, mul_256x256 and fe_reduce512 the device compiles, with sc_mac in C.
ARITH_FORMS = {"host64": (), "limb32": ("-U__SIZEOF_INT128__",)}


@pytest.fixture(scope="module", params=sorted(ARITH_FORMS))
def arith(request, lane):
    if request.param == "host64":
        return lane
    return _build_lane(SO.replace(".so", "_" + request.param + ".so"), ARITH_FORMS[request.param])


@pytest.mark.skipif(not reference_available(), reason="oracle/_ref not built")
def test_lane_schnorr_twist_matches_reference_fixtures(lane):
    """BIP340 on the square-root-free path: the 15 BIP340 vectors and the reference-labelled
    Schnorr tuples (bad keys, off-curve x, R at infinity, odd y(R), mutated s / e)."""
    ts = bip340_vectors() + schnorr_tuples()
    bad = [(t["cls"], t["verdict"]) for t in ts
           if lane.lane_schnorr_verify_twist(t["sig"], t["msg"], t["pub"]) != t["verdict"]]
    assert not bad, bad[:10]


@pytest.mark.skipif(not reference_available(), reason="oracle/_ref not built")
def test_lane_schnorr_signer_vs_reference(lane):
    """The generator's BIP340 signer (synthetic C5 inputs) produces signatures the reference
    accepts, for the x-only key the reference derives."""
    R = Reference()
    rng = random.Random(5)
    for i in range(40):
        d = rng.randrange(1, N).to_bytes(32, "big")
        k = rng.randrange(1, N).to_bytes(32, "big")
        msg = rng.randbytes(32)
        sig, xo = ctypes.create_string_buffer(64), ctypes.create_string_buffer(32)
        assert lane.lane_schnorr_sign(d, msg, k, sig, xo) == 1
        assert R.schnorr_verify(sig.raw, msg, xo.raw) == 1
        assert R.schnorr_sign(d, msg, bytes(32))[1] == xo.raw


TWIST_FORMS = ["lane_verify_twist", "lane_verify_twist_host"]  # SIMT lane code / host engine's form


@pytest.mark.parametrize("fn", TWIST_FORMS)
def test_lane_twist_matches_reference_fixtures(lane, fn):
    """The square-root-free path (csrc/ecdsa_twist.h) on every fixture tuple: compressed keys
    never decompressed, the key's y recovered as -alpha / beta; exceptional classes (R at
    infinity, x(A) == x(B), u1 == 0) take the exact fallback.  Both forms: the kernels' fixed-window
    lane code and the host engine's (wNAF Q half, variable-time inverses)."""
    O = Oracle()
    bad = []
    classes = {}
    for t in ecdsa_tuples():
        tag, x, y = pub_to_tuple(t["pub"])
        ok, r, s = O.der_parse_lax(t["sig"])
        if not ok:
            r = s = bytes(32)
        got = getattr(lane, fn)(tag, x, y, r, s, t["hash"])
        classes[t["cls"]] = classes.get(t["cls"], 0) + 1
        if got != t["verdict"]:
            bad.append((t["cls"], got, t["verdict"]))
    assert not bad, bad[:10]
    assert len(classes) > 10


def _der(r, s):
    def enc(v):
        b = v.to_bytes(32, "big").lstrip(b"\0") or b"\0"
        if b[0] & 0x80:
            b = b"\0" + b
        return b"\x02" + bytes([len(b)]) + b
    body = enc(r) + enc(s)
    return b"\x30" + bytes([len(body)]) + body


@pytest.mark.parametrize("fn", TWIST_FORMS)
def test_lane_twist_random_vs_oracle(lane, fn):
    """Random signed tuples with mutations (flipped key parity, random x -- about half of them
    non-residues --, hybrid / uncompressed encodings, negated y, message and s flips) through
    the square-root-free lane code against the oracle's CPubKey::Verify."""
    O = Oracle()
    rng = random.Random(11)
    P = 2**256 - 2**32 - 977
    bad, seen = [], set()
    for i in range(240):
        d = rng.randrange(1, N)
        msg = rng.randbytes(32)
        qx, qy = (int.from_bytes(b, "big") for b in O.ecmult_gen(d.to_bytes(32, "big")))
        k = rng.randrange(1, N)
        rx = int.from_bytes(O.ecmult_gen(k.to_bytes(32, "big"))[0], "big")
        r = rx % N
        s = pow(k, N - 2, N) * (int.from_bytes(msg, "big") % N + r * d) % N
        mode = i % 8
        comp = mode in (0, 1, 2, 3)
        if mode == 1:
            qy = P - qy                      # flipped parity: the signature is for -Q
        elif mode == 2:
            qx = rng.randrange(P)            # random x: non-residue about half the time
        elif mode == 3 or mode == 6:
            msg = bytes([msg[0] ^ 1]) + msg[1:]
        elif mode == 4:
            s = N - s                        # high s: normalised, still valid
        elif mode == 5:
            qy = P - qy                      # uncompressed, wrong y sign
        if comp:
            pub = bytes([2 + (qy & 1)]) + qx.to_bytes(32, "big")
        else:
            tag = rng.choice([4, 6 + (qy & 1)])
            pub = bytes([tag]) + qx.to_bytes(32, "big") + qy.to_bytes(32, "big")
        exp = O.pubkey_verify(pub, msg, _der(r, s))
        tag, x, y = pub_to_tuple(pub)
        got = getattr(lane, fn)(tag, x, y, r.to_bytes(32, "big"), s.to_bytes(32, "big"), msg)
        seen.add((mode, exp))
        if got != exp:
            bad.append((i, mode, got, exp))
    assert not bad, bad[:10]
    assert {(0, 1), (1, 0), (2, 0), (4, 1), (5, 0), (7, 1)} <= seen


@pytest.mark.skipif(not reference_available(), reason="oracle/_ref not built")
def test_lane_schnorr_twist_random_vs_reference(lane):
    """Random BIP340 signatures (the generator's signer) with mutations -- s, e (message), r,
    the key's x (a non-residue about half the time) -- through the square-root-free lane code
    against the reference's secp256k1_schnorrsig_verify."""
    R = Reference()
    rng = random.Random(23)
    bad, seen = [], set()
    for i in range(160):
        d = rng.randrange(1, N).to_bytes(32, "big")
        k = rng.randrange(1, N).to_bytes(32, "big")
        msg = rng.randbytes(32)
        sig, xo = ctypes.create_string_buffer(64), ctypes.create_string_buffer(32)
        assert lane.lane_schnorr_sign(d, msg, k, sig, xo) == 1
        sig, xo = bytearray(sig.raw), bytearray(xo.raw)
        mode = i % 5
        if mode == 1:
            sig[40] ^= 4
        elif mode == 2:
            msg = bytes([msg[0] ^ 1]) + msg[1:]
        elif mode == 3:
            sig[5] ^= 1
        elif mode == 4:
            xo = bytearray(rng.randbytes(32))
        sig, xo = bytes(sig), bytes(xo)
        exp = R.schnorr_verify(sig, msg, xo)
        got = lane.lane_schnorr_verify_twist(sig, msg, xo)
        seen.add((mode, exp))
        if got != exp:
            bad.append((i, mode, got, exp))
    assert not bad, bad[:10]
    assert (0, 1) in seen and (1, 0) in seen


def test_lane_scalar_mul_inv_mod_n(lane):
    """sc_mul / sc_inv (the mod-n product-scanning reduction) against Python integers: random
    operands, the edge values 0, 1, n - 1, n - 2 and operands just below 2^256 (reduced inputs
    are < n, but the fold must hold for any 512-bit product)."""
    rnd = random.Random(0x5C)
    edge = [0, 1, 2, N - 1, N - 2, (1 << 255), N >> 1, (1 << 256) - 1]
    pairs = [(a, b) for a in edge for b in edge]
    pairs += [(rnd.getrandbits(256), rnd.getrandbits(256)) for _ in range(3000)]
    out = ctypes.create_string_buffer(32)
    for a, b in pairs:
        lane.lane_sc_mul(a.to_bytes(32, "big"), b.to_bytes(32, "big"), out)
        assert int.from_bytes(out.raw, "big") == (a * b) % N, (hex(a), hex(b))
    for _ in range(200):
        a = rnd.randrange(1, N)
        lane.lane_sc_inv(a.to_bytes(32, "big"), out)
        assert int.from_bytes(out.raw, "big") == pow(a, -1, N)


def test_mi30_safegcd_inverse_host(lane):
    """The GPU lanes' inverse (csrc/modinv_device.h, compiled here for the CPU) against
    pow(a, -1, m) for p and n: edge and random operands (the device run is in test_field_gpu)."""
    P = 2**256 - 2**32 - 977
    rng = random.Random(0x30)
    arr = ctypes.c_uint32 * 8
    for m in (P, N):
        minv = pow(m, -1, 2**30)
        vals = [0, 1, 2, 3, m - 1, m - 2, (m + 1) // 2, 2**255 % m, 2**128] + \
            [rng.randrange(m) for _ in range(3000)]
        for a in vals:
            out = arr()
            lane.lane_mi30_inverse(arr(*[(a >> (32 * i)) & 0xFFFFFFFF for i in range(8)]),
                                   arr(*[(m >> (32 * i)) & 0xFFFFFFFF for i in range(8)]),
                                   ctypes.c_uint32(minv), out)
            got = sum(out[i] << (32 * i) for i in range(8))
            assert got == (pow(a, -1, m) if a else 0), (hex(m), hex(a))


# ---------------------------------------------------------------------------------------------
# The device self-test's operand families (scalar_cases.py, test_scalar_gpu.py) on the host builds
# ---------------------------------------------------------------------------------------------
def _pack(vals):
    arr = (ctypes.c_uint32 * (8 * len(vals)))()
    for i, v in enumerate(vals):
        for j in range(8):
            arr[8 * i + j] = (v >> (32 * j)) & 0xFFFFFFFF
    return arr


def _unpack(arr, n):
    return [sum(arr[8 * i + j] << (32 * j) for j in range(8)) for i in range(n)]


def _sc_run(L, op, a_vals, b_vals=None):
    n = len(a_vals)
    out, out2 = (ctypes.c_uint32 * (8 * n))(), (ctypes.c_uint32 * (8 * n))()
    L.lane_sc_selftest.argtypes = [ctypes.c_int] + [ctypes.POINTER(ctypes.c_uint32)] * 4 + \
        [ctypes.c_size_t]
    assert L.lane_sc_selftest(op, _pack(a_vals), _pack(b_vals if b_vals is not None else [0] * n),
                              out, out2, n) == 0
    return _unpack(out, n), _unpack(out2, n)


def test_lane_sc_mul_reduction_carries(arith):
    """sc_mul / sc_sqr over operands whose third fold carries out of 2^256 or lands in
    [n, 2^256) -- the two cases of the first conditional subtraction that random products never
    reach -- with the coverage asserted on the Python model of the folds."""
    import scalar_cases as S
    pairs = S.mul_pairs()
    cov = S.mul_coverage(pairs)
    assert cov["carry"] >= 100 and cov["ge_n"] >= 1000 and cov["q8"] >= {0, 1, 2}, cov
    got, _ = _sc_run(arith, 0, [a for a, _ in pairs], [b for _, b in pairs])
    bad = [(hex(a), hex(b), hex(g)) for (a, b), g in zip(pairs, got) if g != a * b % N]
    assert not bad, f"sc_mul: {len(bad)} mismatches, first {bad[0]}"
    vals = S.sqr_operands()
    cov = S.mul_coverage([(a, a) for a in vals])
    assert cov["carry"] >= 100 and cov["ge_n"] >= 1000 and cov["q8"] >= {0, 1, 2}, cov
    got, _ = _sc_run(arith, 1, vals)
    bad = [(hex(a), hex(g)) for a, g in zip(vals, got) if g != a * a % N]
    assert not bad, f"sc_sqr: {len(bad)} mismatches, first {bad[0]}"


def test_lane_sc_add_neg(arith):
    import scalar_cases as S
    pairs = S.add_pairs()
    sums = [a + b for a, b in pairs]
    assert sum(t >= S.M for t in sums) >= 1000 and sum(N <= t < S.M for t in sums) >= 1000
    assert {N, N - 1, N + 1, S.M, S.M - 1} <= set(sums)
    got, _ = _sc_run(arith, 2, [a for a, _ in pairs], [b for _, b in pairs])
    bad = [(hex(a), hex(b), hex(g)) for (a, b), g in zip(pairs, got) if g != (a + b) % N]
    assert not bad, f"sc_add: {len(bad)} mismatches, first {bad[0]}"
    vals = S.neg_operands()
    got, _ = _sc_run(arith, 3, vals)
    bad = [(hex(a), hex(g)) for a, g in zip(vals, got) if g != -a % N]
    assert not bad, f"sc_neg: {len(bad)} mismatches, first {bad[0]}"


def test_lane_split_lambda(arith):
    """sc_mul_shift_384 and sc_split_lambda against the reference's formula restated on integers,
    k1 + lambda k2 == k, both halves below 2^128 in absolute value; lane_split (the byte-string
    export) agrees with it."""
    import scalar_cases as S
    vals = S.shift_operands()
    for op, g in ((4, S.G1), (5, S.G2)):
        got, _ = _sc_run(arith, op, vals)
        bad = [(hex(k), hex(r)) for k, r in zip(vals, got) if r != S.mul_shift_model(k, g)]
        assert not bad, f"sc_mul_shift_384: {len(bad)} mismatches, first {bad[0]}"
    vals = S.split_operands()
    k1s, k2s = _sc_run(arith, 6, vals)
    bad = []
    for k, k1, k2 in zip(vals, k1s, k2s):
        if (k1, k2) != S.split_model(k) or (k1 + S.LAM * k2) % N != k or \
                abs(S.signed(k1)) >= 2**128 or abs(S.signed(k2)) >= 2**128:
            bad.append((hex(k), hex(k1), hex(k2)))
    assert not bad, f"sc_split_lambda: {len(bad)} mismatches, first {bad[0]}"
    small = S.split_small_pairs()
    assert len(small) == 324
    k1s, k2s = _sc_run(arith, 6, [k for _, _, k in small])
    assert [(S.signed(x), S.signed(y)) for x, y in zip(k1s, k2s)] == [(a, b) for a, b, _ in small]
    o1, o2 = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    for k in vals[:300]:
        arith.lane_split(k.to_bytes(32, "big"), o1, o2)
        assert (int.from_bytes(o1.raw, "big"), int.from_bytes(o2.raw, "big")) == S.split_model(k)


def test_lane_fe_sqrt(arith):
    import scalar_cases as S
    P = S.P
    vals = S.sqrt_operands()
    roots, oks = _sc_run(arith, 7, vals)
    bad = []
    for a, r, ok in zip(vals, roots, oks):
        if r >= P or ok != (1 if r * r % P == a % P else 0) or \
                ok != (1 if pow(a % P, (P - 1) // 2, P) in (0, 1) else 0) or \
                r != pow(a % P, (P + 1) // 4, P):
            bad.append((hex(a), hex(r), ok))
    assert not bad, f"fe_sqrt: {len(bad)} mismatches, first {bad[0]}"


def test_lane_recoding_reconstructs_the_scalar(lane):
    """digit_index (WQ = 4 over an odd 128-bit k) and comb_digit (WC = 16 over an odd 256-bit u1):
    sum d_i 2^(w i) == the scalar, every digit odd and inside its table, the top digit positive;
    the digits equal the closed form.  Integer-only code, so the CPU result stands for the
    device."""
    import scalar_cases as S
    par = (ctypes.c_int * 5)()
    lane.lane_recode_params(par)
    wq, qtab, wc, ctab, cwin = list(par)
    assert (wq, qtab, wc, ctab, cwin) == (4, 8, 16, 32768, 16)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    for fn, w, tab, nwin, nlimb, vals in (
            (lane.lane_recode_q, wq, qtab, 128 // wq, 4, S.recode_q_operands()),
            (lane.lane_recode_comb, wc, ctab, cwin, 8, S.recode_comb_operands())):
        assert {1, 2**128 - 1} <= set(vals) and len(vals) > 1500
        seen_idx = [set() for _ in range(nwin)]
        for k in vals:
            assert k & 1
            limbs = (ctypes.c_uint32 * nlimb)(*[(k >> (32 * i)) & 0xFFFFFFFF for i in range(nlimb)])
            d = (ctypes.c_int32 * nwin)()
            ix = (ctypes.c_uint32 * nwin)()
            assert fn(ctypes.cast(limbs, u32p), d, ix) == nwin
            ds = list(d)
            assert sum(v << (w * i) for i, v in enumerate(ds)) == k, hex(k)
            assert all(v & 1 and abs(v) < 2 * tab and 0 <= j < tab for v, j in zip(ds, ix)), hex(k)
            assert ds[-1] > 0 and ds == S.recode_model(k, w, nwin), hex(k)
            for s, j in zip(seen_idx, ix):
                s.add(j)
        # both table extremes in every window below the top
        assert all({0, tab - 1} <= s for s in seen_idx[:-1])


# ---------------------------------------------------------------------------------------------
# The structured-scalar fixture (tests/golden/structured_scalars.npz) through the host lane forms
# ---------------------------------------------------------------------------------------------
def test_structured_fixture_holds_what_its_generator_promises():
    """The committed file's header (coverage asserted at generation time on the Python model of
    the split and the recodings): a stale or cut file fails here."""
    from fixtures import structured_scalars
    f = structured_scalars()
    h = f["header"]
    assert h["flag_combinations"] == 16 and h["zero_halves"] == [0, 1]
    assert h["q_indices"] == [list(range(8))] * 2 and h["comb_extremes_every_window"]
    assert h["fold_carry_rows"] >= 30 and h["u1_zero_rows"] >= 1
    assert len(f["ecdsa"]) == 2 * h["ecdsa_rows"] and h["ecdsa_rows"] >= 3000
    assert len(f["tweak"]) == 2 * h["tweak_rows"] and len(f["schnorr"]) == h["schnorr_rows"]
    assert sum(t["verdict"] for t in f["ecdsa"]) == h["ecdsa_valid"] + h["ecdsa_twin_valid"]
    classes = {t["cls"] for t in f["ecdsa"]}
    assert {"u1_zero", "u1_pow2", "u1_window", "u1_window_even", "u2_glv", "u2_lambda",
            "reduce_carry", "reduce_below_nc", "a_equals_b", "a_equals_minus_b_s1"} <= classes


@pytest.mark.parametrize("fn", TWIST_FORMS)
def test_lane_twist_structured_scalars(lane, fn):
    """Every ECDSA row of the structured-scalar fixture and its invalid twin through both host
    forms of the lane code."""
    from fixtures import structured_scalars
    f = getattr(lane, fn)
    bad = []
    for i, t in enumerate(structured_scalars()["ecdsa"]):
        tag, x, y = pub_to_tuple(t["pub"])
        if f(tag, x, y, t["r32"], t["s32"], t["hash"]) != t["verdict"]:
            bad.append((i, t["cls"], t["verdict"]))
    assert not bad, (len(bad), bad[:10])


def test_lane_schnorr_exceptional(arith):
    """tests/golden/schnorr_exceptional.npz through both host builds of the lane code: s = +-e d
    takes schnorr_twist_exceptional through x(A) == x(B) (R at infinity, the doubling)."""
    from fixtures import schnorr_exceptional
    bad = [(i, t["cls"], t["verdict"]) for i, t in enumerate(schnorr_exceptional())
           if arith.lane_schnorr_verify_twist(t["sig"], t["msg"], t["pub"]) != t["verdict"]]
    assert not bad, (len(bad), bad[:10])


def test_lane_schnorr_structured_scalars(lane):
    from fixtures import structured_scalars
    bad = [(i, t["cls"], t["verdict"]) for i, t in enumerate(structured_scalars()["schnorr"])
           if lane.lane_schnorr_verify_twist(t["sig"], t["msg"], t["pub"]) != t["verdict"]]
    assert not bad, (len(bad), bad[:10])
