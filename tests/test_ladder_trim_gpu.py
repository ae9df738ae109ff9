"""GPU: the trimmed ladders (the affine + affine first addition of the Q ladder and the comb, the
signed Q-table read) on every kernel that runs them.

1,024 ECDSA rows and 1,024 BIP340 rows drawn class by class from the fixtures (valid rows, the
adversarial classes of ecdsa_tuples.npz / schnorr_tuples.npz / schnorr_exceptional.npz, the
structured-scalar classes: comb digits at the table's extremes, zero GLV halves, corrections
through infinity, u1 == 0, x(A) == x(B)) against their golden verdicts (the reference's):

  * alone, at most one wave per SIMD           twist_keyq2_kernel (the half ladders)
  * scattered in a batch above cus * 128 rows  twist_keyq_kernel + twist_ladder_g_kernel
  * that batch in three chunks                 ecdsa_tprep_kernel + twist_ladder_kernel<false>
  * the BIP340 rows in one launch              schnorr_tladder_kernel

and one 300-row C2 workload through Workload.run, unmutated (valid by construction) and with a
tenth of its items mutated (against the reference's interpreter where it is built)."""
import random

import pytest

from fixtures import (bip340_vectors, ecdsa_tuples, pub_to_tuple, schnorr_exceptional, schnorr_tuples,
                      structured_scalars)
from oracle_ctypes import Oracle, Reference, reference_available

pytestmark = pytest.mark.gpu

ROWS = 1024


def _by_class(rows, n, seed):
    """n rows, taken class by class in turn so that every class is in."""
    rng = random.Random(seed)
    groups = {}
    for t in rows:
        groups.setdefault(t["cls"], []).append(t)
    for g in groups.values():
        rng.shuffle(g)
    out = []
    while len(out) < n:
        for c in sorted(groups):
            if groups[c] and len(out) < n:
                out.append(groups[c].pop())
    assert len(groups) <= n
    rng.shuffle(out)
    return out


def _verify_tuples(batch):
    import bitcoinconsensus_amd as B
    return B.ecdsa_verify_tuples(*(b"".join(t[k] for t in batch)
                                   for k in ("pub65", "hash", "r32", "s32")))


@pytest.fixture(scope="module")
def ecdsa_rows():
    O = Oracle()

    def row(t):
        tag, x, y = pub_to_tuple(t["pub"])
        if "r32" in t:
            r, s = t["r32"], t["s32"]
        else:
            ok, r, s = O.der_parse_lax(t["sig"])
            if not ok:
                r = s = bytes(32)
        return dict(t, pub65=bytes([tag]) + x + y, r32=r, s32=s)

    old = ecdsa_tuples()
    every = structured_scalars()["ecdsa"] + old
    rows = [row(t) for t in _by_class(every, ROWS, 0x7A1)]
    fill = [row(t) for t in old if t["cls"].startswith("valid_") and t["verdict"] == 1][:256]
    assert {t["cls"] for t in rows} == {t["cls"] for t in every}
    assert 100 < sum(t["verdict"] for t in rows) < ROWS - 100  # valid and invalid rows mix
    return rows, fill


def _bad(rows, got):
    return [(t["cls"], i, g, t["verdict"]) for i, (t, g) in enumerate(zip(rows, got))
            if g != t["verdict"]]


def test_ecdsa_rows_half_ladders(ecdsa_rows):
    """At most one wave per SIMD: twist_keyq2_kernel runs twist_accumulate_q_half."""
    import bitcoinconsensus_amd as B
    rows, _ = ecdsa_rows
    assert 2 * len(rows) <= B.blib().mi_device_cus(0) * 256
    bad = _bad(rows, _verify_tuples(rows))
    assert not bad, (len(bad), bad[:20])


def test_ecdsa_rows_throughput_and_chunked_kernels(ecdsa_rows):
    """The rows scattered among valid ones in a batch above the latency threshold
    (twist_keyq_kernel + twist_ladder_g_kernel), then the same batch in three chunks
    (ecdsa_tprep_kernel + twist_ladder_kernel<false>): the golden verdicts, and the same bytes."""
    import bitcoinconsensus_amd as B
    rows, fill = ecdsa_rows
    n = B.blib().mi_device_cus(0) * 128 + 4096 + 77  # above the threshold, no multiple of a wave
    rng = random.Random(0x7A2)
    pos = sorted(rng.sample(range(n), len(rows)))
    batch = [fill[rng.randrange(len(fill))] for _ in range(n)]
    for p, t in zip(pos, rows):
        batch[p] = t
    one = _verify_tuples(batch)
    bad = _bad(rows, [one[p] for p in pos])
    assert not bad, (len(bad), bad[:20])
    assert sum(one) == sum(t["verdict"] for t in rows) + n - len(rows)
    lanes = (n // 3) & ~255
    B.set_chunk_lanes(lanes)
    try:
        three = _verify_tuples(batch)
    finally:
        B.set_chunk_lanes(0)
    assert three == one


def test_schnorr_rows():
    """1,024 BIP340 rows through schnorr_tladder_kernel."""
    import bitcoinconsensus_amd as B
    every = structured_scalars()["schnorr"] + schnorr_tuples() + bip340_vectors() + schnorr_exceptional()
    rows = _by_class(every, ROWS, 0x7A3)
    assert {t["cls"] for t in rows} == {t["cls"] for t in every}
    assert 100 < sum(t["verdict"] for t in rows) < ROWS - 100
    got = B.schnorr_verify_tuples(*(b"".join(t[k] for t in rows) for k in ("sig", "msg", "pub")))
    bad = _bad(rows, got)
    assert not bad, (len(bad), bad[:20])


def test_c2_workload_300_rows():
    """A 300-row C2 workload through Workload.run: every generated spend verifies; with a tenth of
    the items mutated, every tuple's verdict is the reference interpreter's for that check."""
    import bitcoinconsensus_amd as B
    from test_workload_gpu import SEED, mutate
    n = 300
    w = B.Workload(n, seed=SEED)
    try:
        w.run()
        assert list(w.verdicts()) == [1] * n and w.tuple_items() == list(range(n))
        items = [w.item(i) for i in range(n)]
    finally:
        w.free()
    rng = random.Random(0x7A4)
    kinds = {}
    for i in range(n):
        if rng.random() < 0.10:
            items[i] = mutate(rng, items[i])[:4]
            kinds[i] = True
    w = B.Workload(kind="items", items=items)
    try:
        w.run()
        v, ti, msgs = w.verdicts(), w.tuple_items(), w.msgs()
    finally:
        w.free()
    for t, i in enumerate(ti):
        if i not in kinds:
            assert v[t] == 1, i
    assert sum(1 for t, i in enumerate(ti) if v[t] == 0) >= 3  # rejections happen on the GPU
    if not reference_available():
        return
    R = Reference()
    for t, i in enumerate(ti):
        if i not in kinds:
            continue
        r, _, recs = R.capture_script(*items[i], B.VERIFY_ALL)
        pair = (msgs[32 * t: 32 * t + 32], v[t])
        ref_pairs = [(c["sighash"], c["verdict"]) for c in recs]
        # a key that no longer hashes to its program: the reference stopped before the check
        assert pair in ref_pairs or (not recs and r == 0 and pair[1] == 0), i
