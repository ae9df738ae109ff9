"""GPU: whole Taproot inputs through the product C ABI (bcc_taproot_spend_batch: the host pass of
csrc/host/taproot_spend.cpp and the fused device round of csrc/taproot_commit.hip: commitment
kernels, the leaf-copy kernel, the SigMsg / TapSighash / BIP340 kernels on one stream) against the
committed reference answers, the wave / workgroup / inversion-group edges of the batch size, round
boundaries, the device list, and fresh random spends labelled by the live reference.

As in test_taproot_spend_host.py, class s_* (signature) cases have no reference whole-spend verdict:
their expectation is the entry point's rule applied to the reference's per-check answers."""
import random

import pytest

import bitcoinconsensus_amd as B
import taproot_spend_cases as S
from oracle_ctypes import Reference, reference_available
from test_taproot_spend_host import check_cases

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 4099]


@pytest.fixture(scope="module")
def golden():
    return S.load_golden()


@pytest.fixture(scope="module")
def pool(golden):
    """A mixed pool (key path, every script template, class R cases, mutations; short txs) and
    what each item gives when it is the only one of its call, on the kernels."""
    cases = [c for c in golden if len(c["tx"]) < 1200]
    B.set_host_small_round(0)  # a batch of one reaches the kernels
    one = [B.taproot_spend_batch(S.items_of([c]))[0] for c in cases]
    return cases, one


def test_spend_golden_cases_on_gpu(golden):
    B.set_host_small_round(0)
    check_cases(B.taproot_spend_batch(S.items_of(golden)), golden)


def test_spend_single_calls_match_reference(pool):
    cases, one = pool
    check_cases(one, cases)
    kinds = {c["cls"].split("_")[1] for c in cases}
    assert {"keypath", "checksig", "verify", "multi", "mutate", "control", "weight"} <= kinds, kinds


@pytest.mark.parametrize("n", SIZES)
def test_spend_batch_sizes_equal_single_calls(pool, n):
    cases, one = pool
    rng = random.Random(n)
    idx = [rng.randrange(len(cases)) for _ in range(n)]
    B.set_host_small_round(0)
    assert B.taproot_spend_batch(S.items_of([cases[i] for i in idx])) == [one[i] for i in idx]


def big_batch(pool, golden):
    cases, one = pool
    by_id = {id(c): o for c, o in zip(cases, one)}
    rng = random.Random(4099)
    pick = [rng.choice(cases) for _ in range(4095)]
    multi = [c for c in golden if c["cls"].startswith("s_multi_input")][:4]
    assert len(multi) == 4 and len({id(c["tx"]) for c in multi}) == 1
    pick[998:998] = multi  # one tx's four inputs across the cut at 1000
    assert len(pick) == 4099
    return pick, [by_id.get(id(c), c["expected"]) for c in pick]


def test_spend_round_boundaries(pool, golden):
    pick, want = big_batch(pool, golden)
    items = S.items_of(pick)
    B.set_host_small_round(0)
    assert B.taproot_spend_batch(items) == want
    try:
        B.set_spend_round(1000)  # five rounds over three slots
        assert B.taproot_spend_batch(items) == want
    finally:
        B.set_spend_round(0)


@pytest.mark.parametrize("round_items", [1, 3, 8])
def test_spend_rounds_without_device_work_between_rounds_with(pool, round_items):
    """Runs of items the host decides alone (an empty witness, a wrong control size, a size-rule
    failure on the key path: no commitment, no signature check) between signed items, cut into
    small rounds: whole rounds then launch nothing, and the rounds around them still get their
    own slots' verdicts.  Equal to the single-item calls."""
    cases, one = pool
    host = [i for i, c in enumerate(cases) if c["cls"].startswith(("r_witness_empty", "r_control_size",
                                                                   "r_keypath_sig_", "r_program_"))]
    dev = [i for i, c in enumerate(cases) if c["cls"].startswith("s_") and c["expected"] != (1, 0)
           and c["expected"][1] in (39, 46)]
    dev += [i for i, c in enumerate(cases) if c["cls"].startswith("s_") and c["expected"] == (1, 0)]
    assert len(host) >= 10 and len(dev) >= 40
    rng = random.Random(round_items)
    idx = []
    while len(idx) < 600:
        idx += [rng.choice(dev) for _ in range(rng.randrange(1, 2 * round_items + 2))]
        idx += [rng.choice(host) for _ in range(rng.randrange(round_items, 4 * round_items + 1))]
    want = [one[i] for i in idx]
    assert (1, 0) in want and (0, 46) in want
    B.set_host_small_round(0)
    try:
        B.set_spend_round(round_items)
        assert B.taproot_spend_batch(S.items_of([cases[i] for i in idx])) == want
    finally:
        B.set_spend_round(0)


def test_spend_device_list(pool, golden):
    pick, want = big_batch(pool, golden)
    B.set_host_small_round(0)
    try:
        B.set_devices([0, 0, 0])
        assert B.taproot_spend_batch(S.items_of(pick), device=-1) == want
    finally:
        B.set_devices([])


def test_spend_small_batches_on_the_host_lanes(pool):
    """At most bcc_set_host_small_round() items: the commitments on the host lane code."""
    cases, one = pool
    try:
        B.set_host_small_round(16)
        for lo in range(0, len(cases), 16):
            assert B.taproot_spend_batch(S.items_of(cases[lo:lo + 16])) == one[lo:lo + 16]
    finally:
        B.set_host_small_round(0)


def test_spend_leaf_copy_indexing(golden):
    """Every script-path item has two or more queued checks and some items have none (key path is
    absent on purpose: rows and commitment lanes then never line up by accident): a check's leaf
    hash must come from its own spend's lane."""
    multi = [c for c in golden if len(c.get("checks", [])) >= 2 and c["checks"][0]["leaf"] is not None]
    none = [c for c in golden if c["cls"] in ("r_success_start", "r_checkmultisig", "r_eval_false",
                                              "r_control_size_34_true", "r_mutate_p_true",
                                              "r_leaf_version_c2", "r_witness_empty_1")]
    assert len(multi) >= 10 and len(none) == 7
    rng = random.Random(77)
    pick = [rng.choice(multi if rng.random() < 0.6 else none) for _ in range(700)]
    B.set_host_small_round(0)
    check_cases(B.taproot_spend_batch(S.items_of(pick)), pick)


@pytest.mark.skipif(not reference_available(), reason="needs the reference build (oracle/_ref)")
def test_spend_random_cases_against_live_reference():
    cases = S.random_cases(Reference(), random.Random(0xC0FFEE), 400)
    valid = sum(c["expected"] == (1, 0) for c in cases)
    assert 0.3 * len(cases) <= valid <= 0.7 * len(cases), valid
    errs = {c["expected"][1] for c in cases}
    assert S.LISTED_ERRORS <= errs, S.LISTED_ERRORS - errs
    B.set_host_small_round(0)
    check_cases(B.taproot_spend_batch(S.items_of(cases)), cases)
