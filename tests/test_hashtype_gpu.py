"""GPU: the device paths for the remaining ECDSA-era hash types (bcc_set_device_hashtypes): legacy
NONE / SINGLE / ANYONECANPAY through legacy_in_kernel (K_lin) and the table-only role of the front
kernel, BIP143 SIGHASH_SINGLE through bip143_in_kernel (csrc/sighash.hip).  The sweeps and goldens
of hashtype_cases.py through bcc_debug_sighash must equal the model byte for byte with the switch
on, and with it off (the host-preimage path K1 / K2 / K3 the switch bypasses); the signed fixture
through bitcoinconsensus_verify_batch must give the reference's (ret, err) under every staging
mode.  test_hashtype_host.py asserts what the sweeps cover."""
import gzip
import json
import os
import random

import pytest

import bitcoinconsensus_amd as B
import hashtype_cases as H
import sighash_model as M
from test_hashtype_host import spends

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SETS = ["legacy_rawtx", "bip143_single_rawtx", "golden_legacy", "golden_random"]


def the_set(name):
    if name.startswith("golden_"):
        checks, exp = H.golden_checks(name[len("golden_"):])
        return checks, None, exp
    return H.sweep(name)


@pytest.fixture
def switch_on():
    B.set_device_hashtypes(True)
    yield
    B.set_device_hashtypes(False)


@pytest.mark.parametrize("name", SETS)
def test_gpu_digests_with_the_switch_on(name, switch_on):
    checks, geoms, exp = the_set(name)
    got = B.debug_sighash(checks)
    msg = H.mismatches(name, got, exp, geoms)
    assert not msg, msg
    k = B.last_sighash_kinds()
    assert k["host_preimage"] == 0, k
    assert k["legacy_rawtx"] + k["single_bug"] == len(H.legacy_non_all(checks)), k
    assert k["bip143_rawtx_single"] == sum(1 for c in checks if c[5] == 1 and c[3] & 0x1f == 3), k


def test_gpu_old_and_new_job_kinds_share_a_round(switch_on):
    """One call with everything shuffled together with legacy SIGHASH_ALL template jobs and the
    other BIP143 types: K_wtx's hashing and table-only roles, K3', K_win and K_lin in one round,
    transactions with jobs of several kinds."""
    checks, exp, gs = [], [], []
    for name in SETS:
        c, g, e = the_set(name)
        checks += c
        exp += e
        gs += g if g else [dict(set=name)] * len(c)
    for name in ("legacy_all", "bip143"):
        c, g, e = M.family(name)
        checks += c[::7]
        exp += e[::7]
        gs += g[::7]
    order = list(range(len(checks)))
    random.Random(H.SEED).shuffle(order)
    got = B.debug_sighash([checks[i] for i in order])
    msg = H.mismatches("everything, shuffled", got, [exp[i] for i in order], [gs[i] for i in order])
    assert not msg, msg
    k = B.last_sighash_kinds()
    assert k["legacy_template"] > 0 and k["bip143_rawtx"] > 0 and k["legacy_rawtx"] > 0, k


@pytest.mark.parametrize("name", ["legacy_rawtx", "bip143_single_rawtx"])
def test_gpu_digests_with_the_switch_off(name):
    """The same sweeps on the host-preimage path (K1 / K2 / K3), which the switch bypasses."""
    B.set_device_hashtypes(False)
    checks, geoms, exp = the_set(name)
    got = B.debug_sighash(checks)
    msg = H.mismatches(name + ", switch off", got, exp, geoms)
    assert not msg, msg
    k = B.last_sighash_kinds()
    assert k["legacy_rawtx"] == 0 and k["bip143_rawtx_single"] == 0 and k["host_preimage"] > 0, k


MODES = {
    "default": (lambda: None, lambda: None),
    "pinned_image": (lambda: B.set_direct_upload(False), lambda: B.set_direct_upload(True)),
    "chunks_of_60": (lambda: B.set_pipeline_chunk(60), lambda: B.set_pipeline_chunk(500000)),
    "host_threads_4": (lambda: B.set_host_threads(4), lambda: B.set_host_threads(0)),
    "devices_0_0": (lambda: B.set_devices([0, 0]), lambda: B.set_devices([])),
}


@pytest.fixture(scope="module")
def fixture_off():
    """The fixture through verify_batch with the switch off, once."""
    items, flags, tuples = spends()
    B.set_device_hashtypes(False)
    rc, res = B.verify_batch_raw(tuples, flags)
    assert rc >= 0
    return res


@pytest.mark.parametrize("mode", list(MODES))
def test_gpu_signed_fixture_through_verify_batch(mode, fixture_off):
    items, flags, tuples = spends()
    exp = [(it["ret"], it["err"]) for it in items]
    enter, leave = MODES[mode]
    enter()
    B.set_device_hashtypes(True)
    try:
        rc, res = B.verify_batch_raw(tuples, flags)
        k = B.last_sighash_kinds()
    finally:
        B.set_device_hashtypes(False)
        leave()
    assert rc == sum(r for r, _ in exp)
    bad = [(i, items[i]["kind"], hex(items[i]["hashtype"]), items[i]["mutation"], res[i], exp[i])
           for i in range(len(items)) if res[i] != exp[i]]
    assert not bad, bad[:10]
    assert res == fixture_off
    assert k["legacy_rawtx"] > 0 and k["bip143_rawtx_single"] > 0 and k["host_preimage"] == 0, k


def test_gpu_long_chains_still_go_to_the_host(switch_on):
    """200 inputs signed with NONE: 129-block chains.  With bcc_set_host_chain_blocks(8) the host
    hashes them during the device round as before; with the default (160) they are K_lin lanes."""
    d = json.load(gzip.open(os.path.join(GOLDEN, "hashtype_spends.json.gz")))
    tx = bytes.fromhex(d["long_none"]["tx"])
    its = d["long_none"]["items"]
    tuples = [(bytes.fromhex(it["spk"]), it["amount"], tx, it["nin"]) for it in its]
    exp = [(it["ret"], it["err"]) for it in its]
    assert len(its) == 200 and all(r == 1 for r, _ in exp)
    B.set_host_chain_blocks(8)
    try:
        rc, res = B.verify_batch_raw(tuples, d["flags"])
        k = B.last_sighash_kinds()
    finally:
        B.set_host_chain_blocks(B.HOST_CHAIN_BLOCKS_DEFAULT)
    assert res == exp
    assert k["host_hashed"] == 200 and k["legacy_rawtx"] == 0 and k["host_preimage"] == 0, k
    rc, res = B.verify_batch_raw(tuples, d["flags"])
    k = B.last_sighash_kinds()
    assert res == exp
    assert k["legacy_rawtx"] == 200 and k["host_hashed"] == 0, k
