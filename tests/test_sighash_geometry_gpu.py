"""GPU: the byte-geometry sweeps of sighash_model.py through the device sighash kernels
(csrc/sighash.hip): sighash_front_kernel (K1 aux messages, K3' sha256d_tpl_lane, K_wtx
bip143_tx_lane), bip143_in_kernel, patch_digests_kernel and sha256d_msgs_kernel by way of
bcc_debug_sighash, taproot_tx_kernel and taproot_msg_kernel by way of bcc_taproot_verify_batch.
Every digest must equal the hashlib model's byte for byte; test_sighash_geometry.py pins the model
against the reference and asserts what the sweeps cover."""
import random

import pytest

import bitcoinconsensus_amd as B
import sighash_model as M

pytestmark = pytest.mark.gpu

FAMILIES = list(M.ECDSA_FAMILIES)


@pytest.mark.parametrize("name", FAMILIES)
def test_gpu_sighash_matches_model_on_family(name):
    checks, _, _ = M.family(name)
    msg = M.mismatches(name, B.debug_sighash(checks))
    assert not msg, msg


def test_gpu_sighash_matches_model_all_families_shuffled():
    """One call with every family, shuffled: a wave mixes lanes of different trip counts and
    geometries, and the three lane roles of the front kernel share workgroups."""
    checks, exp, gs = [], [], []
    for name in FAMILIES:
        c, g, e = M.family(name)
        checks += c
        exp += e
        gs += [dict(x, family=name) for x in g]
    order = list(range(len(checks)))
    random.Random(M.SEED).shuffle(order)
    got = B.debug_sighash([checks[i] for i in order])
    msg = M.mismatches("all families, shuffled", got, [exp[i] for i in order], [gs[i] for i in order])
    assert not msg, msg


def test_gpu_sighash_tx_order_and_shuffled_agree():
    """Whole transactions in input order (consecutive lanes = consecutive inputs of one tx, as in
    production) and the same checks shuffled give identical digests."""
    checks, gs, exp = M.family("legacy_tx_order")
    ordered = B.debug_sighash(checks)
    order = list(range(len(checks)))
    random.Random(M.SEED + 99).shuffle(order)
    shuffled = B.debug_sighash([checks[i] for i in order])
    back = [None] * len(checks)
    for at, i in enumerate(order):
        back[i] = shuffled[at]
    assert back == ordered, [(i, gs[i]) for i in range(len(checks)) if back[i] != ordered[i]][:10]
    msg = M.mismatches("legacy_tx_order", ordered)
    assert not msg, msg


def test_gpu_tapsighash_matches_model():
    checks, gs, _ = M.family("taproot")
    out, hs = B.taproot_verify_batch(checks, sighashes=True)
    refused = [(i, gs[i]) for i, (r, _) in enumerate(out) if r == -1]
    assert not refused, refused[:10]
    msg = M.mismatches("taproot", hs)
    assert not msg, msg
