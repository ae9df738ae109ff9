"""Operand families and Python-integer models for the mod-n scalar arithmetic, the GLV split, the
signed odd-window recodings and fe_sqrt (csrc/secp256k1_device.h, ecdsa_lane.h, ecdsa_twist.h).
Shared by the device self-test (test_scalar_gpu.py) and the host builds of the same lane code
(test_lane_host.py), so both see the same operands.

Random operands never reach the last steps of sc_reduce512.  With NC = 2^256 - n (129 bits) the
reduction folds 2^256 == NC three times and then subtracts n at most twice; the value s after the
third fold is congruent to the product and below 2^256 + 2^133, so

    s >= 2^256        (the `carry` handed to the first sc_cond_sub_n)  needs  a b mod n < 2^133,
    n <= s < 2^256    (the first subtraction fires without a carry)    needs  a b mod n < NC,

about 2^-123 each for random products.  The constructed families below choose the residue first:
a random, b = rho a^-1 mod n with rho below NC or just above it.  fold_model() restates the three
folds on integers; the tests assert their coverage conditions on it, never on the code under
test."""
import functools
import random

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
M = 2**256
NC = M - N
LAM = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
G1 = 0x3086D221A7D46BCDE86C90E49284EB153DAA8A1471E8CA7FE893209A45DBB031
G2 = 0xE4437ED6010E88286F547FA90ABFE4C4221208AC9DF506C61571B4AE8AC47F71
MB1 = 0xE4437ED6010E88286F547FA90ABFE4C3                                    # -b1
MB2 = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFE8A280AC50774346DD765CDA83DB1562C    # -b2 mod n

SC_EDGES = [0, 1, 2, N - 1, N - 2, N, N + 1, 2**255, 2**256 - 1, NC, NC - 1, NC + 1, (N + 1) // 2]


# ---------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------
def fold_model(t):
    """The three folds of sc_reduce512 on a 512-bit integer: (s, q8) with s the value after the
    third fold (before the conditional subtractions) and q8 the third fold's multiplier."""
    m = (t % M) + (t >> 256) * NC
    assert m < 2**386
    q = (m % M) + (m >> 256) * NC
    assert q < 2**260
    s = (q % M) + (q >> 256) * NC
    assert s < M + 2**133 and s % N == t % N
    return s, q >> 256


def mul_coverage(pairs):
    """Counts over the model: products whose s carries out of 2^256, products with n <= s < 2^256,
    and the set of third-fold multipliers."""
    carry = ge_n = 0
    q8 = set()
    for a, b in pairs:
        s, q = fold_model(a * b)
        carry += s >= M
        ge_n += N <= s < M
        q8.add(q)
    return dict(carry=carry, ge_n=ge_n, q8=q8)


def split_model(k):
    """scalar_split_lambda restated: c1 = round(k g1 / 2^384), c2 = round(k g2 / 2^384),
    k2 = c1 (-b1) + c2 (-b2), k1 = k - lambda k2, all mod n."""
    c1 = (k * G1 + 2**383) >> 384
    c2 = (k * G2 + 2**383) >> 384
    k2 = (c1 * MB1 + c2 * MB2) % N
    k1 = (k - LAM * k2) % N
    return k1, k2


def mul_shift_model(k, g):
    return (k * g + 2**383) >> 384


def signed(v):
    """The representative of v mod n in (-n/2, n/2]."""
    return v if v <= N - v else v - N


def sqrt_mod_n(a):
    """A square root of a mod n by Tonelli-Shanks (n == 1 mod 4: n - 1 = 2^6 odd), or None."""
    a %= N
    if a == 0:
        return 0
    if pow(a, (N - 1) // 2, N) != 1:
        return None
    q, e = N - 1, 0
    while q % 2 == 0:
        q //= 2
        e += 1
    z = 2
    while pow(z, (N - 1) // 2, N) != N - 1:
        z += 1
    c, x, t = pow(z, q, N), pow(a, (q + 1) // 2, N), pow(a, q, N)
    while t != 1:
        i, u = 0, t
        while u != 1:
            u = u * u % N
            i += 1
        b = pow(c, 1 << (e - i - 1), N)
        x, t, c, e = x * b % N, t * b * b % N, b * b % N, i
    assert x * x % N == a
    return x


def recode_model(k, w, nwin):
    """Signed odd fixed-window digits of an odd k < 2^(w nwin): d_i = 2 ((k >> (w i + 1)) mod 2^w)
    + 1 - 2^w below the top window, d_top = 2 (k >> (w top + 1)) + 1."""
    top = nwin - 1
    ds = [2 * ((k >> (w * i + 1)) & ((1 << w) - 1)) + 1 - (1 << w) for i in range(top)]
    return ds + [2 * (k >> (w * top + 1)) + 1]


# ---------------------------------------------------------------------------------------------
# operand families
# ---------------------------------------------------------------------------------------------
_PICK = [0, 1, 2**32 - 1, 2**32 - 2, 0xFFFFFC2F, None, None]


def limbmix(rng):
    """test_field_gpu.py's recipe: limbs from {0, 1, 2^32 - 1, 2^32 - 2, p's low limb, random};
    all-ones limbs drive the flagged carries of the exact product columns."""
    return sum((rng.getrandbits(32) if (c := rng.choice(_PICK)) is None else c) << (32 * i)
               for i in range(8))


# residue ranges of the constructed families (rho = a b mod n)
RESIDUE_FAMILIES = [("below_nc", 0, NC), ("nc_2nc", NC, 2 * NC), ("nc_plus_2_130", NC, NC + 2**130)]


def constructed_pairs(rng, lo, hi, count):
    out = []
    for _ in range(count):
        a = rng.randrange(1, N)
        out.append((a, rng.randrange(lo, hi) * pow(a, -1, N) % N))
    return out


@functools.lru_cache(maxsize=None)
def mul_pairs(constructed=3000, nrand=3000, nmix=6000, seed=0x5CA1):
    """sc_mul operands (any 256-bit values), edge lanes shuffled among random lanes."""
    rng = random.Random(seed)
    pairs = [(a, b) for a in SC_EDGES for b in SC_EDGES]
    pairs += [(rng.randrange(N), rng.randrange(N)) for _ in range(nrand)]
    pairs += [(rng.getrandbits(256), rng.getrandbits(256)) for _ in range(nrand)]
    pairs += [(limbmix(rng), limbmix(rng)) for _ in range(nmix)]
    for _, lo, hi in RESIDUE_FAMILIES:
        pairs += constructed_pairs(rng, lo, hi, constructed)
    rng.shuffle(pairs)
    return tuple(pairs)


@functools.lru_cache(maxsize=None)
def sqr_operands(constructed=3000, nrand=3000, nmix=3000, seed=0x5CA2):
    """sc_sqr operands: roots of residues drawn from the constructed ranges (where one exists),
    both roots, plus edge, random and limb-mix operands."""
    rng = random.Random(seed)
    vals = list(SC_EDGES)
    vals += [rng.randrange(N) for _ in range(nrand)] + [rng.getrandbits(256) for _ in range(nrand)]
    vals += [limbmix(rng) for _ in range(nmix)]
    for _, lo, hi in RESIDUE_FAMILIES:
        got = 0
        while got < constructed:
            x = sqrt_mod_n(rng.randrange(lo, hi))
            if x is None:
                continue
            vals += [x, N - x]
            got += 2
    rng.shuffle(vals)
    return tuple(vals)


@functools.lru_cache(maxsize=None)
def add_pairs(nrand=2000, seed=0x5CA3):
    """sc_add operands, both below n (its contract): sums at or above 2^256, sums in [n, 2^256),
    the sums n, n +- 1, 2^256 and 2^256 - 1 exactly, and 0, 1, n - 1 against everything."""
    rng = random.Random(seed)
    small = [0, 1, 2, N - 1, N - 2, (N + 1) // 2, (N - 1) // 2, NC, NC - 1, NC + 1, 2**255]
    pairs = [(a, b) for a in small for b in small]
    for _ in range(nrand):
        a = rng.randrange(NC + 2, N)
        pairs.append((a, rng.randrange(M - a, N)))              # a + b >= 2^256
        pairs.append((a, N + rng.randrange(NC) - a))            # n <= a + b < 2^256
        pairs.append((rng.randrange(N), rng.randrange(N)))
        pairs.append((rng.randrange(2**255), rng.randrange(2**255 - NC)))   # no reduction at all
    for _ in range(200):
        a = rng.randrange(NC + 2, N)
        for total in (N, N - 1, N + 1, M, M - 1, M + 1, 2 * N - 2 - rng.randrange(4)):
            b = total - a
            if 0 <= b < N:
                pairs.append((a, b))
    assert all(0 <= a < N and 0 <= b < N for a, b in pairs)
    rng.shuffle(pairs)
    return tuple(pairs)


@functools.lru_cache(maxsize=None)
def neg_operands(nrand=2000, seed=0x5CA4):
    rng = random.Random(seed)
    vals = [0, 1, 2, N - 1, N - 2, (N + 1) // 2, (N - 1) // 2, NC, 2**255, 2**128, 2**32, 2**32 - 1]
    vals += [rng.randrange(N) for _ in range(nrand)]
    vals += [limbmix(rng) % N for _ in range(nrand)]
    rng.shuffle(vals)
    return tuple(vals)


SPLIT_SMALL = [0, 1, -1, 2, -2, 3, 15, 16, -16, 17, 2**64, -(2**64) + 1, 2**100 - 1, 2**120,
               2**124, -(2**124), 2**125 + 1, 2**126 - 1]


def split_small_pairs():
    """(a, b, k = a + lambda b mod n): the model returns (a, b) unchanged for |a|, |b| <= 2^126."""
    return [(a, b, (a + LAM * b) % N) for a in SPLIT_SMALL for b in SPLIT_SMALL]


@functools.lru_cache(maxsize=None)
def split_operands(nrand=4000, nround=500, seed=0x5CA5):
    """sc_split_lambda / sc_mul_shift_384 operands below n: edges, a + lambda b for small signed
    a, b, the rounding edges of both constants (the smallest k whose product reaches
    j 2^384 + 2^383, and k - 1), random values."""
    rng = random.Random(seed)
    vals = [0, 1, 2, N - 1, N - 2, LAM, N - LAM, LAM + 1, LAM - 1, (N + 1) // 2, 2**128,
            2**128 - 1, 2**255]
    vals += [k for _, _, k in split_small_pairs()]
    for g in (G1, G2):
        for _ in range(nround):
            j = rng.randrange((g * N) >> 384)
            k = -(-(j * 2**384 + 2**383) // g)
            assert mul_shift_model(k, g) == j + 1 and mul_shift_model(k - 1, g) == j
            vals += [v for v in (k, k - 1) if 0 <= v < N]
    vals += [rng.randrange(N) for _ in range(nrand)]
    rng.shuffle(vals)
    return tuple(vals)


@functools.lru_cache(maxsize=None)
def shift_operands(nrand=2000, seed=0x5CA6):
    """sc_mul_shift_384 takes any 256-bit value: the split operands plus values at and above n."""
    rng = random.Random(seed)
    vals = list(split_operands()) + [N, N + 1, M - 1, M - 2]
    vals += [rng.getrandbits(256) for _ in range(nrand)] + [limbmix(rng) for _ in range(nrand)]
    rng.shuffle(vals)
    return tuple(vals)


@functools.lru_cache(maxsize=None)
def sqrt_operands(nrand=1500, seed=0x5CA7):
    """fe_sqrt operands (weak, any value below 2^256): 0, 1, residues and non-residues (p == 3 mod
    4, so -x^2 is one), p - 1, weak values in [p, 2^256), limb-mix values."""
    rng = random.Random(seed)
    vals = [0, 1, 2, 3, 4, 7, P - 1, P - 2, P - 4, P, P + 1, P + 2, P + 3, P + 4, M - 1, M - 2,
            (P + 1) // 2, (P - 1) // 2]
    for _ in range(nrand):
        x = rng.randrange(1, P)
        vals += [x * x % P, P - x * x % P, rng.randrange(P)]
    vals += [P + rng.randrange(M - P) for _ in range(300)]
    vals += [limbmix(rng) for _ in range(nrand)]
    rng.shuffle(vals)
    return tuple(vals)


@functools.lru_cache(maxsize=None)
def recode_q_operands(nrand=1000, seed=0x5CA8):
    """Odd 128-bit scalars for digit_index (WQ = 4, 32 windows): 1, 2^128 - 1, 2^k +- 1, every
    window all-zeros or all-ones with the rest random, random values."""
    return _recode_operands(128, 4, nrand, seed, M)


@functools.lru_cache(maxsize=None)
def recode_comb_operands(nrand=1000, seed=0x5CA9):
    """Odd 256-bit scalars below n for comb_digit (WC = 16, 16 windows), same families."""
    return _recode_operands(256, 16, nrand, seed, N)


def _recode_operands(bits, w, nrand, seed, bound):
    rng = random.Random(seed)
    vals = [1, 3, 2**bits - 1, 2**128 - 1]
    for k in range(1, bits):
        vals += [2**k + 1, 2**k - 1]
    for win in range(bits // w):
        mask = ((1 << w) - 1) << (w * win)
        # the window a digit reads starts one bit up (d_i comes from bits w i + 1 .. w i + w)
        mask1 = (mask << 1) & (2**bits - 1)
        for _ in range(8):
            r = rng.getrandbits(bits)
            vals += [r & ~mask, r | mask, r & ~mask1, r | mask1]
    vals += [rng.getrandbits(bits) for _ in range(nrand)]
    vals += [N - 2 - 2 * i for i in range(4)] if bits == 256 else []
    vals = [v | 1 for v in vals]
    vals = [v for v in vals if v < bound and v < 2**bits]
    rng.shuffle(vals)
    return tuple(vals)
