"""GPU: the adversarial fixtures through EVERY ladder kernel, not only the latency mode.

A batch with 2 n <= cus * 256 goes to twist_keyq2_kernel (launch_keyq, csrc/ecdsa_verify.hip), so
the fixture files, fed in one small batch each, never reached the throughput kernels.  Here the
structured-scalar fixture (tests/golden/structured_scalars.npz: chosen u1 / u2 -- comb digits at
the table's extremes, GLV halves equal to zero, corrections through infinity, the mod-n reduction's
carries) and the older ecdsa_tuples.npz / schnorr_tuples.npz go, scattered among valid filler rows
so that waves mix, through

  1. small batches                          twist_keyq2_kernel
  2. one batch of more than cus * 128 rows  twist_keyq_kernel + twist_ladder_g_kernel
  3. the same batch in >= 3 chunks          ecdsa_tprep_kernel + twist_ladder_kernel<false>
  4. pubkey_verify_batch on that batch      K_der and the engine's staging in front of them
  5. BIP340 rows in one and in three chunks schnorr_tladder_kernel
  6. tweak rows                             tweak_add_kernel (the comb alone)

and every fixture row is compared with its golden verdict (the reference's)."""
import random

import pytest

from fixtures import (bip340_vectors, ecdsa_tuples, pub_to_tuple, schnorr_exceptional, schnorr_tuples,
                      structured_scalars)
from oracle_ctypes import Oracle

pytestmark = pytest.mark.gpu


def _cus():
    import bitcoinconsensus_amd as B
    cus = B.blib().mi_device_cus(0)
    assert cus > 0
    return cus


def _mismatches(rows, pos, got):
    return [(t["cls"], i, got[p], t["verdict"]) for i, (t, p) in enumerate(zip(rows, pos))
            if got[p] != t["verdict"]]


@pytest.fixture(scope="module")
def ecdsa_rows():
    """Fixture rows (structured scalars with their twins, then ecdsa_tuples.npz) and valid filler
    rows, each as (pub, hash, der sig, tag || x || y, r32, s32)."""
    O = Oracle()

    def row(t):
        tag, x, y = pub_to_tuple(t["pub"])
        if "r32" in t:
            r, s = t["r32"], t["s32"]
        else:
            ok, r, s = O.der_parse_lax(t["sig"])  # checker-side parse for the raw tuple ABI
            if not ok:
                r = s = bytes(32)
        return dict(t, pub65=bytes([tag]) + x + y, r32=r, s32=s)

    old = ecdsa_tuples()
    rows = [row(t) for t in structured_scalars()["ecdsa"] + old]
    fill = [row(t) for t in old if t["cls"].startswith("valid_") and t["verdict"] == 1]
    assert len(rows) > 9000 and len(fill) >= 500
    return rows, fill


def _scatter(rows, fill, n, seed):
    """n rows: `rows` at random positions (in order), valid filler rows everywhere else."""
    assert n >= len(rows)
    rng = random.Random(seed)
    pos = sorted(rng.sample(range(n), len(rows)))
    batch = [fill[rng.randrange(len(fill))] for _ in range(n)]
    for p, t in zip(pos, rows):
        batch[p] = t
    return batch, pos


def _verify_tuples(batch):
    import bitcoinconsensus_amd as B
    return B.ecdsa_verify_tuples(*(b"".join(t[k] for t in batch)
                                   for k in ("pub65", "hash", "r32", "s32")))


@pytest.fixture(scope="module")
def large(ecdsa_rows):
    """The large batch: more than cus * 128 rows (49,152 on a 256-CU MI355X), so launch_keyq takes
    the throughput kernel; its filler rows must all verify."""
    rows, fill = ecdsa_rows
    cus = _cus()
    n = max(cus * 192, len(rows) + len(rows) // 4)
    assert 2 * n > cus * 4 * 64
    batch, pos = _scatter(rows, fill, n, 0xC0FFEE)
    return batch, pos


@pytest.fixture(scope="module")
def large_one_chunk(large):
    return _verify_tuples(large[0])


def test_small_batches_latency_kernel(ecdsa_rows):
    """Path 1: batches of at most cus * 128 rows (twist_keyq2_kernel)."""
    rows, fill = ecdsa_rows
    cap = _cus() * 128
    n = len(rows) + len(rows) // 4
    batch, pos = _scatter(rows, fill, n, 0xBA7C4)
    got = b"".join(_verify_tuples(batch[i:i + cap]) for i in range(0, n, cap))
    bad = _mismatches(rows, pos, got)
    assert not bad, (len(bad), bad[:20])
    assert sum(got) == sum(t["verdict"] for t in rows) + n - len(rows)


def test_large_batch_throughput_kernels(ecdsa_rows, large, large_one_chunk):
    """Path 2: one batch above the latency threshold (twist_keyq_kernel + twist_ladder_g_kernel)."""
    rows, _ = ecdsa_rows
    batch, pos = large
    bad = _mismatches(rows, pos, large_one_chunk)
    assert not bad, (len(bad), bad[:20])
    assert sum(large_one_chunk) == sum(t["verdict"] for t in rows) + len(batch) - len(rows)


def test_large_batch_chunked_kernels(ecdsa_rows, large, large_one_chunk):
    """Path 3: the same batch in at least three chunks (ecdsa_tprep_kernel + twist_ladder_kernel):
    the golden verdicts again, and byte-identical to the one-chunk run."""
    import bitcoinconsensus_amd as B
    rows, _ = ecdsa_rows
    batch, pos = large
    lanes = (len(batch) // 3) & ~255
    assert lanes >= 256 and 3 * lanes <= len(batch)
    B.set_chunk_lanes(lanes)
    try:
        got = _verify_tuples(batch)
    finally:
        B.set_chunk_lanes(0)
    bad = _mismatches(rows, pos, got)
    assert not bad, (len(bad), bad[:20])
    assert got == large_one_chunk


def test_large_batch_pubkey_verify_batch(ecdsa_rows, large, large_one_chunk):
    """Path 4: CPubKey::Verify level (lax DER on the GPU in front of the same kernels)."""
    import bitcoinconsensus_amd as B
    rows, _ = ecdsa_rows
    batch, pos = large
    got = B.pubkey_verify_batch([(t["pub"], t["hash"], t["sig"]) for t in batch])
    bad = _mismatches(rows, pos, got)
    assert not bad, (len(bad), bad[:20])
    assert got == large_one_chunk


def test_schnorr_one_and_three_chunks():
    """Path 5: BIP340 rows (structured keys / nonces / s, schnorr_tuples.npz, the BIP340 vectors,
    the s = +-e d rows of schnorr_exceptional.npz) among valid rows, in one schnorr_tladder_kernel
    launch and in three."""
    import bitcoinconsensus_amd as B
    old = schnorr_tuples()
    rows = structured_scalars()["schnorr"] + old + bip340_vectors() + schnorr_exceptional()
    fill = [t for t in old if t["cls"] == "valid" and t["verdict"] == 1]
    assert len(rows) > 2000 and len(fill) >= 300
    lanes = 1280
    n = 3 * lanes - 37  # three chunks, the last one short and no multiple of the workgroup
    batch, pos = _scatter(rows, fill, n, 0x5C40)
    args = [b"".join(t[k] for t in batch) for k in ("sig", "msg", "pub")]
    one = B.schnorr_verify_tuples(*args)
    B.set_chunk_lanes(lanes)
    try:
        three = B.schnorr_verify_tuples(*args)
    finally:
        B.set_chunk_lanes(0)
    bad = _mismatches(rows, pos, one)
    assert not bad, (len(bad), bad[:20])
    assert three == one
    assert sum(one) == sum(t["verdict"] for t in rows) + n - len(rows)


def test_tweak_rows_through_the_comb():
    """Path 6: the comb's scalar families as tweaks through tweak_add_kernel, rows and twins among
    valid rows."""
    import bitcoinconsensus_amd as B
    rows = structured_scalars()["tweak"]
    fill = [t for t in rows if t["verdict"] == 1 and t["cls"].startswith("t_window")]
    assert len(rows) > 4000 and len(fill) >= 100
    n = len(rows) + 1500 + 19
    batch, pos = _scatter(rows, fill, n, 0x7EA4)
    got = B.xonly_tweak_check_tuples(b"".join(t["q"] for t in batch),
                                     bytes(t["parity"] for t in batch),
                                     b"".join(t["p"] for t in batch),
                                     b"".join(t["t"] for t in batch))
    bad = _mismatches(rows, pos, got)
    assert not bad, (len(bad), bad[:20])
    assert sum(got) == sum(t["verdict"] for t in rows) + n - len(rows)
