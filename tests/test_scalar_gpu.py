"""Device mod-n scalar arithmetic (csrc/secp256k1_device.h: the exact product columns behind
sc_mul / sc_sqr, the inline-asm sc_mac folds of sc_reduce512 and its two conditional subtractions,
sc_add, sc_neg, sc_mul_shift_384, sc_split_lambda) and fe_sqrt against Python integers, exactly.
Operands come from scalar_cases.py: edge lanes are shuffled among random lanes, so a wave that
takes a rare branch also carries lanes that must pass through it unchanged.  Coverage conditions
are asserted on the Python model of the folds, never on the device output."""
import ctypes

import pytest

import scalar_cases as S
from scalar_cases import G1, G2, LAM, M, N, P


def pack(vals):
    arr = (ctypes.c_uint32 * (8 * len(vals)))()
    for i, v in enumerate(vals):
        for j in range(8):
            arr[8 * i + j] = (v >> (32 * j)) & 0xFFFFFFFF
    return arr


def unpack(arr, n):
    return [sum(arr[8 * i + j] << (32 * j) for j in range(8)) for i in range(n)]


def run(op, a_vals, b_vals=None):
    from bitcoinconsensus_amd import blib
    L = blib()
    n = len(a_vals)
    a = pack(a_vals)
    b = pack(b_vals if b_vals is not None else [0] * n)
    out = (ctypes.c_uint32 * (8 * n))()
    out2 = (ctypes.c_uint32 * (8 * n))()
    assert L.mi_sc_selftest(op, a, b, out, out2, n) == 0
    return unpack(out, n), unpack(out2, n)


def test_mul_operands_reach_the_reduction_carries():
    """The model's coverage of the sc_mul operand list (no GPU): the counts the device test relies
    on, several times over."""
    cov = S.mul_coverage(S.mul_pairs())
    assert cov["carry"] >= 100, cov
    assert cov["ge_n"] >= 1000, cov
    assert cov["q8"] >= {0, 1, 2}, cov
    roots = S.sqr_operands()
    cov = S.mul_coverage([(a, a) for a in roots])
    assert cov["carry"] >= 100 and cov["ge_n"] >= 1000 and cov["q8"] >= {0, 1, 2}, cov


@pytest.mark.gpu
def test_sc_mul_matches_integers():
    pairs = S.mul_pairs()
    cov = S.mul_coverage(pairs)
    assert cov["carry"] >= 100 and cov["ge_n"] >= 1000 and cov["q8"] >= {0, 1, 2}, cov
    got, _ = run(0, [a for a, _ in pairs], [b for _, b in pairs])
    bad = [(hex(a), hex(b), hex(g)) for (a, b), g in zip(pairs, got) if g != a * b % N]
    assert not bad, f"sc_mul: {len(bad)} mismatches, first {bad[0]}"


@pytest.mark.gpu
def test_sc_sqr_matches_integers():
    vals = S.sqr_operands()
    cov = S.mul_coverage([(a, a) for a in vals])
    assert cov["carry"] >= 100 and cov["ge_n"] >= 1000 and cov["q8"] >= {0, 1, 2}, cov
    got, _ = run(1, vals)
    bad = [(hex(a), hex(g)) for a, g in zip(vals, got) if g != a * a % N]
    assert not bad, f"sc_sqr: {len(bad)} mismatches, first {bad[0]}"


@pytest.mark.gpu
def test_sc_add_and_neg_match_integers():
    pairs = S.add_pairs()
    sums = [a + b for a, b in pairs]
    assert sum(t >= M for t in sums) >= 1000 and sum(N <= t < M for t in sums) >= 1000
    assert {N, N - 1, N + 1, M, M - 1} <= set(sums)
    got, _ = run(2, [a for a, _ in pairs], [b for _, b in pairs])
    bad = [(hex(a), hex(b), hex(g)) for (a, b), g in zip(pairs, got) if g != (a + b) % N]
    assert not bad, f"sc_add: {len(bad)} mismatches, first {bad[0]}"
    vals = S.neg_operands()
    assert {0, 1, N - 1} <= set(vals)
    got, _ = run(3, vals)
    bad = [(hex(a), hex(g)) for a, g in zip(vals, got) if g != -a % N]
    assert not bad, f"sc_neg: {len(bad)} mismatches, first {bad[0]}"


@pytest.mark.gpu
@pytest.mark.parametrize("op,g", [(4, G1), (5, G2)], ids=["g1", "g2"])
def test_sc_mul_shift_384_matches_integers(op, g):
    vals = S.shift_operands()
    got, _ = run(op, vals)
    bad = [(hex(k), hex(r)) for k, r in zip(vals, got) if r != S.mul_shift_model(k, g)]
    assert not bad, f"sc_mul_shift_384: {len(bad)} mismatches, first {bad[0]}"


@pytest.mark.gpu
def test_sc_split_lambda_matches_reference_formula():
    vals = S.split_operands()
    k1s, k2s = run(6, vals)
    bad = []
    for k, k1, k2 in zip(vals, k1s, k2s):
        if (k1, k2) != S.split_model(k) or (k1 + LAM * k2) % N != k or \
                abs(S.signed(k1)) >= 2**128 or abs(S.signed(k2)) >= 2**128:
            bad.append((hex(k), hex(k1), hex(k2)))
    assert not bad, f"sc_split_lambda: {len(bad)} mismatches, first {bad[0]}"
    # small signed halves come back unchanged (zero in either half included)
    small = S.split_small_pairs()
    k1s, k2s = run(6, [k for _, _, k in small])
    assert [(S.signed(x), S.signed(y)) for x, y in zip(k1s, k2s)] == [(a, b) for a, b, _ in small]


@pytest.mark.gpu
def test_fe_sqrt_matches_integers():
    vals = S.sqrt_operands()
    res = [v for v in vals if pow(v % P, (P - 1) // 2, P) == 1]
    assert len(res) >= 1000 and len(vals) - len(res) >= 1000
    assert {0, 1, P - 1, P, M - 1} <= set(vals) and sum(v >= P for v in vals) >= 300
    roots, oks = run(7, vals)
    bad = []
    for a, r, ok in zip(vals, roots, oks):
        if r >= P or ok != (1 if r * r % P == a % P else 0) or \
                ok != (1 if pow(a % P, (P - 1) // 2, P) in (0, 1) else 0) or \
                r != pow(a % P, (P + 1) // 4, P):
            bad.append((hex(a), hex(r), ok))
    assert not bad, f"fe_sqrt: {len(bad)} mismatches, first {bad[0]}"
