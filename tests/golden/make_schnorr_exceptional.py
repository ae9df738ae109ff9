"""Generate tests/golden/schnorr_exceptional.npz (run where the reference build oracle/_ref exists):

    python3 tests/golden/make_schnorr_exceptional.py

BIP340 rows whose final sum R = s G - e P is exceptional: x(s G) == x(e P).  The challenge
e = H(rx || P || m) does not depend on s, so for a key with known secret d (even y), a message and
any rx -- here the x of a random point -- s can be chosen after e:

  s_eq_ed        s = e d      s G == e P: R is the point at infinity
  s_eq_minus_ed  s = -e d     s G == -e P: the sum is a doubling, R = -2 e P
  */nb           s + 1 or s - 1 of the row before it (alternating): the sum next to the exceptional
                 one, through the ordinary addition
  valid_same_key a valid signature under the same key and message

Keys: the structured secrets of make_structured_scalars.py's BIP340 rows plus random ones.  Every
verdict comes from the REFERENCE (secp256k1_schnorrsig_verify); the integer model py_schnorr is
asserted to agree with it, and s G == +-e P is asserted on the model for the two classes.  The
counts go to the file's header."""
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import commit_cases as C  # noqa: E402
from make_fixtures import tagged_hash  # noqa: E402
from make_structured_scalars import LAM, N, P, mul, py_schnorr  # noqa: E402
from oracle_ctypes import Reference  # noqa: E402

OUT = os.path.join(HERE, "schnorr_exceptional.npz")
STRUCTURED_KEYS = [1, 2, 3, 7, N - 1, N - 2, LAM, N - LAM, LAM + 1, 2**128, 2**127 + 1, 2**255]
RANDOM_KEYS, MESSAGES_PER_KEY = 28, 2


def challenge(rx, px, msg):
    return int.from_bytes(tagged_hash(b"BIP0340/challenge", C.b32(rx) + C.b32(px) + msg), "big") % N


def main():
    R = Reference()
    rng = random.Random(0xE8CE97)
    rows = []  # (cls, d_even, px, sig, msg)
    for ki, d in enumerate(STRUCTURED_KEYS + [rng.randrange(1, N) for _ in range(RANDOM_KEYS)]):
        pt = mul(d)
        de = d if pt[1] % 2 == 0 else N - d  # the secret of the even-y lift of x(P)
        px = pt[0]
        for mi in range(MESSAGES_PER_KEY):
            msg = rng.choice([bytes(32), b"\xff" * 32, rng.randbytes(32), rng.randbytes(32)])
            rx = mul(rng.randrange(1, N))[0]
            e = challenge(rx, px, msg)
            assert e != 0
            eP = mul(e * de)
            step = 1 if (ki + mi) & 1 else -1
            for cls, s in (("s_eq_ed", e * de % N), ("s_eq_minus_ed", -e * de % N)):
                sG = mul(s)
                if cls == "s_eq_ed":
                    assert sG == eP
                else:
                    assert sG == (eP[0], P - eP[1])
                rows.append((cls, de, px, C.b32(rx) + C.b32(s), msg))
                rows.append((cls + "/nb", de, px, C.b32(rx) + C.b32((s + step) % N), msg))
            k = rng.randrange(1, N)
            Rp = mul(k)
            if Rp[1] & 1:
                k = N - k
            s = (k + challenge(Rp[0], px, msg) * de) % N
            rows.append(("valid_same_key", de, px, C.b32(Rp[0]) + C.b32(s), msg))
    n = len(rows)
    classes = sorted({r[0] for r in rows})
    out = dict(sig=np.zeros((n, 64), np.uint8), msg=np.zeros((n, 32), np.uint8),
               pub=np.zeros((n, 32), np.uint8), verdict=np.zeros(n, np.uint8),
               cls=np.zeros(n, np.uint8))
    counts = {c: 0 for c in classes}
    for i, (cls, de, px, sig, msg) in enumerate(rows):
        v = R.schnorr_verify(sig, msg, C.b32(px))
        assert v == py_schnorr(de, px, sig, msg), (cls, i)
        assert v == (1 if cls == "valid_same_key" else 0), (cls, i, v)
        out["sig"][i] = np.frombuffer(sig, np.uint8)
        out["msg"][i] = np.frombuffer(msg, np.uint8)
        out["pub"][i] = np.frombuffer(C.b32(px), np.uint8)
        out["verdict"][i] = v
        out["cls"][i] = classes.index(cls)
        counts[cls] += 1
    header = dict(rows=n, valid=int(out["verdict"].sum()), counts=counts,
                  keys=len(STRUCTURED_KEYS) + RANDOM_KEYS, structured_keys=len(STRUCTURED_KEYS))
    np.savez_compressed(OUT, **out, classes=np.array(classes), header=np.array(json.dumps(header)))
    print(json.dumps(header))
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
