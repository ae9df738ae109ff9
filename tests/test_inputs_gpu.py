"""GPU: any input against its spent outputs through the product C ABI (bcc_verify_inputs_batch:
the routing of csrc/host/inputs.cpp in front of the ECDSA engine's sighash + ECDSA kernels and the
Taproot engine's commitment, SigMsg / TapSighash and BIP340 kernels) against the committed reference
answers of tests/mixed_input_cases.py, the wave / workgroup edges of the batch size with both kinds
in one batch, round cuts on both sides at once, the device list, the host lanes, and fresh random
mixed transactions labelled by the live reference."""
import random

import pytest

import bitcoinconsensus_amd as B
import mixed_input_cases as M
from oracle_ctypes import Oracle, Reference, reference_available
from test_inputs_host import CLASSES, check, pool_cases, run_batches

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 4099]
F = M.ALL | M.TAPROOT


@pytest.fixture(scope="module")
def pool():
    """Mixed, golden and contract cases (short txs) and what each gives when it is the only item
    of its call, on the kernels."""
    cases = [c for c in pool_cases() if len(c["tx"]) < 1200]
    B.set_host_small_round(0)  # a batch of one reaches the kernels
    one = [B.verify_inputs_batch([dict(tx=c["tx"], spent=c["spent"], nin=c["nin"])], F)[0] for c in cases]
    return cases, one


@pytest.mark.parametrize("name", list(CLASSES))
def test_golden_class_as_batches_on_gpu(name):
    B.set_host_small_round(0)
    cases = CLASSES[name]()
    check(run_batches(cases, stats=True), cases)


def test_single_calls_match_reference(pool):
    cases, one = pool
    check(one, cases)
    assert {c["cls"].split(":")[0] for c in cases} >= {"mixed", "tr", "lifted_tr", "v1", "ecdsa"}


@pytest.mark.parametrize("n", SIZES)
def test_batch_sizes_equal_single_calls(pool, n):
    cases, one = pool
    rng = random.Random(n)
    idx = [rng.randrange(len(cases)) for _ in range(n)]
    B.set_host_small_round(0)
    assert B.verify_inputs_batch(M.items_of([cases[i] for i in idx]), F) == [one[i] for i in idx]


def sides(pool):
    cases, one = pool
    v1 = [i for i, c in enumerate(cases) if c["v1"]]
    ec = [i for i, c in enumerate(cases) if not c["v1"] and c["expected"][1] == 0]
    assert len(v1) > 100 and len(ec) > 100
    return cases, one, v1, ec


def test_kinds_alternating_item_by_item(pool):
    """v1, non-v1, v1, ...: every run of the partition has length one, so a scatter or gather index
    that is off by one lands on an item of the other kind."""
    cases, one, v1, ec = sides(pool)
    rng = random.Random(257)
    idx = [rng.choice(v1 if k % 2 == 0 else ec) for k in range(257)]
    B.set_host_small_round(0)
    assert B.verify_inputs_batch(M.items_of([cases[i] for i in idx]), F) == [one[i] for i in idx]
    st = B.last_inputs_stats()
    assert (st["taproot_side_items"], st["ecdsa_side_items"], st["host_decided_items"]) == (129, 128, 0)


@pytest.mark.parametrize("side", ["v1", "non_v1"])
def test_one_sided_batches(pool, side):
    cases, one, v1, ec = sides(pool)
    rng = random.Random(65)
    idx = [rng.choice(v1 if side == "v1" else ec) for _ in range(300)]
    B.set_host_small_round(0)
    assert B.verify_inputs_batch(M.items_of([cases[i] for i in idx]), F) == [one[i] for i in idx]
    st = B.last_inputs_stats()
    assert (st["taproot_side_items"], st["ecdsa_side_items"]) == ((300, 0) if side == "v1" else (0, 300))


CHUNK = 150


def big_batch(pool):
    """4,099 items around one transaction's four inputs, two of each kind: 999 v1 items and
    CHUNK - 1 items of the ECDSA side come before them in any order, so its two v1 inputs are items
    999 and 1,000 of the Taproot side (across the cut of set_spend_round(1000)) and its two other
    inputs items CHUNK - 1 and CHUNK of the ECDSA side (where set_pipeline_chunk(CHUNK) would cut;
    the engine keeps one transaction's adjacent inputs in one chunk, so the cut moves past them)."""
    cases, one, v1, ec = sides(pool)
    by_id = {id(c): o for c, o in zip(cases, one)}
    rng = random.Random(4099)
    head = [cases[rng.choice(v1)] for _ in range(999)] + [cases[rng.choice(ec)] for _ in range(CHUNK - 1)]
    rng.shuffle(head)
    four = next(t for t in M.mixed_txs() if sorted(i["kind"] in M.V1_KINDS for i in t["inputs"]) ==
                [False, False, True, True])
    tail = [rng.choice(cases) for _ in range(4099 - len(head) - 4)]
    pick = head + M.cases_of_tx(four) + tail
    return pick, [by_id.get(id(c), c["expected"]) for c in pick]


def test_round_cuts_on_both_sides_at_once(pool):
    pick, want = big_batch(pool)
    assert len(pick) == 4099
    items = M.items_of(pick)
    B.set_host_small_round(0)
    assert B.verify_inputs_batch(items, F) == want
    st = B.last_inputs_stats()
    assert st["ecdsa_side_items"] >= 3 * CHUNK + 2 and st["taproot_side_items"] > 2000
    try:
        B.set_spend_round(1000)
        B.set_pipeline_chunk(CHUNK)
        assert B.verify_inputs_batch(items, F) == want
    finally:
        B.set_pipeline_chunk(500_000)
        B.set_spend_round(0)


def test_device_list(pool):
    pick, want = big_batch(pool)
    B.set_host_small_round(0)
    try:
        B.set_devices([0, 0, 0])
        # twice the batch: more than 4,096 v1 items, so the Taproot side is really spread
        assert B.verify_inputs_batch(M.items_of(pick) * 2, F) == want * 2
        assert B.last_inputs_stats()["taproot_side_items"] > 4096
    finally:
        B.set_devices([])


def test_small_mixed_batches_on_the_host_lanes(pool):
    """At most bcc_set_host_small_round() items: both sides on the host lane code."""
    cases, one = pool
    rng = random.Random(16)
    idx = [rng.randrange(len(cases)) for _ in range(480)]
    try:
        B.set_host_small_round(16)
        for lo in range(0, len(idx), 16):
            sub = idx[lo:lo + 16]
            assert B.verify_inputs_batch(M.items_of([cases[i] for i in sub]), F) == [one[i] for i in sub]
    finally:
        B.set_host_small_round(0)


@pytest.mark.skipif(not reference_available(), reason="needs the reference build (oracle/_ref)")
def test_random_mixed_inputs_against_live_reference():
    # 4 inputs in 10 tampered: one tamper often leaves the transaction's other inputs valid
    txs = M.random_mixed_txs(Reference(), Oracle(), random.Random(0xD1CE), 400, tamper_rate=0.4)
    cases = [c for t in txs for c in M.cases_of_tx(t, "random")]
    assert len(cases) >= 400
    valid = sum(c["expected"] == (1, 0) for c in cases)
    assert 0.3 * len(cases) <= valid <= 0.7 * len(cases), valid
    assert {c["cls"].split(":")[1] for c in cases} == set(M.KINDS)
    B.set_host_small_round(0)
    check(B.verify_inputs_batch(M.items_of(cases), F), cases)
    assert B.last_inputs_stats()["taproot_side_items"] == sum(c["v1"] for c in cases)
