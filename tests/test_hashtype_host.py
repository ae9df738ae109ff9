"""CPU: the device paths for the remaining ECDSA-era hash types (bcc_set_device_hashtypes) as far
as they go without a GPU: the ABI, what the sweeps of hashtype_cases.py cover, the job builder
(engine.cpp add_sighash_job: LinJob, the SIGHASH_SINGLE WinJob) with the product's host
evaluation of those jobs (host_verify.cpp host_sighash, which host small rounds and the
device-failure fallback run), and the whole engine over the signed fixture with every round on
that host path.  test_hashtype_gpu.py runs the same cases through the kernels."""
import ctypes
import gzip
import json
import os

import pytest

import hashtype_cases as H
import sighash_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEADER = os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "bcc_amd.h")


def test_abi_declares_the_switch_and_the_counts():
    text = open(HEADER).read()
    assert "int bcc_set_device_hashtypes(int on);" in text
    assert "void bcc_last_sighash_kinds(bcc_sighash_kinds* out);" in text
    assert "Results never\n * depend on it." in text or "Results never depend on it." in text
    E, _ = H.host_lib()
    assert E.bcc_set_device_hashtypes(0) == 0
    k = H.Kinds()
    E.bcc_last_sighash_kinds(ctypes.byref(k))
    import bitcoinconsensus_amd as B
    assert [f for f, _ in B.SighashKinds._fields_] == list(H.KIND_FIELDS)
    assert callable(B.set_device_hashtypes) and callable(B.last_sighash_kinds)


def test_legacy_sweep_covers_every_edge():
    """A condition on the inputs, from the geometry records alone."""
    _, geoms, _ = H.sweep("legacy_rawtx")
    live = [g for g in geoms if not g["single_bug"]]
    classes = {c for _, c in H.BASE_TYPES}
    have = {(g["cls"], g["pre_len"] % 64) for g in live}
    missing = [(c, r) for c in sorted(classes) for r in H.RESIDUES if (c, r) not in have]
    assert not missing, missing
    # every compactsize crossing: the input count, SINGLE's count of nin + 1 outputs, the code
    # field, an output script and a skipped scriptSig, on both sides
    non_acp = [g for g in live if g["cls"] in ("none", "single")]
    assert {1, 3} <= {g["in_count_cs"] for g in non_acp}
    assert {252, 253, 254} <= {g["nin"] for g in non_acp}
    assert {1, 3} <= {g["single_count_cs"] for g in live if g["single_count_cs"]}
    assert {252, 253} <= {g["k"] + 1 for g in live if g["single_count_cs"]}
    for cls in classes:
        assert {252, 253, 254} <= {g["code_len"] for g in live if g["cls"] == cls}, cls
    assert any(g["seps"] for g in live) and any(g["seps"] == 2 and g["code_len"] >= 252 for g in live)
    assert {0, 25, 252, 253} <= {n for g in live for n in g["out_lens"]}
    assert {0, 5, 107, 253} <= {n for g in live for n in g["sig_lens"]}
    # the SINGLE bug beside the last valid index, both wire forms, all three uploads
    bug = {(g["nin"], g["k"], g["nout"]) for g in geoms if g["single_bug"]}
    ok = {(g["nin"], g["k"], g["nout"]) for g in live if g["cls"].startswith("single")}
    for nin in (2, 3, 5, 252, 253, 254):
        assert (nin, nin - 1, nin) in ok and (nin, nin - 1, 1) in bug, nin
    assert {(g["witness"], g["stripped"]) for g in live} == {(False, False), (True, True), (True, False)}
    assert {0, 1} <= {g["nout"] for g in live}
    assert {g["ht"] for g in geoms} >= {h & 0xffffffff for h, _ in H.BASE_TYPES + H.GARBAGE_TYPES}
    for nin in (1, 2, 3, 5, 252, 253, 254):
        assert {0, nin // 2, nin - 1} <= {g["k"] for g in geoms if g["nin"] == nin}, nin


def test_bip143_single_sweep_covers_every_edge():
    _, geoms, _ = H.sweep("bip143_single_rawtx")
    assert {g["ht"] for g in geoms} == {3, 0x83}
    assert {55, 56, 64} <= {g["out_len"] for g in geoms if g["out_len"]}
    assert {8 + 1 + 0, 8 + 1 + 252, 8 + 3 + 253} <= {g["out_len"] for g in geoms if g["out_len"]}
    assert any(not g["has_output"] and g["nout"] == 0 for g in geoms)
    assert any(not g["has_output"] and g["nout"] > 0 for g in geoms)
    assert {g["pre_len"] % 64 for g in geoms} >= set(H.RESIDUES)


def _sets():
    out = {name: H.sweep(name) for name in H.SWEEPS}
    for name in ("legacy", "random"):
        checks, exp = H.golden_checks(name)
        out["golden_" + name] = (checks, None, exp)
    return out


@pytest.mark.parametrize("name", ["legacy_rawtx", "bip143_single_rawtx", "golden_legacy",
                                  "golden_random"])
def test_job_builder_and_host_evaluation(name):
    checks, geoms, exp = _sets()[name]
    if name == "golden_legacy":
        assert len(checks) == 500
    if name == "golden_random":
        assert len(checks) == 1200
    non_all = H.legacy_non_all(checks)
    single143 = [c for c in checks if c[5] == 1 and c[3] & 0x1f == 3]
    got_on, kinds_on, bytes_on = H.host_sighash(checks, True)
    msg = H.mismatches(name + ", switch on", got_on, exp, geoms)
    assert not msg, msg
    assert kinds_on["host_preimage"] == 0, kinds_on
    assert kinds_on["legacy_rawtx"] + kinds_on["single_bug"] == len(non_all), kinds_on
    assert kinds_on["bip143_rawtx_single"] == len(single143), kinds_on
    assert kinds_on["host_hashed"] == 0, kinds_on
    assert sum(kinds_on.values()) == len(checks), kinds_on
    bugs = sum(1 for (tx, _, k, ht, _, sv), e in zip(checks, exp) if sv == 0 and ht & 0x1f == 3
               and e == M.ONE)
    assert kinds_on["single_bug"] == bugs, (kinds_on, bugs)

    got_off, kinds_off, bytes_off = H.host_sighash(checks, False)
    msg = H.mismatches(name + ", switch off", got_off, exp, geoms)
    assert not msg, msg
    assert kinds_off["legacy_rawtx"] == 0 and kinds_off["bip143_rawtx_single"] == 0, kinds_off
    assert kinds_off["host_preimage"] > 0, kinds_off
    assert kinds_off["host_preimage"] == len(non_all) - bugs + len(single143), kinds_off
    assert kinds_off["single_bug"] == bugs
    for f in ("legacy_template", "bip143_rawtx"):
        assert kinds_on[f] == kinds_off[f], (f, kinds_on, kinds_off)


def test_one_transaction_many_checks_uploads_it_once_per_check_set():
    """A 200-input transaction signed with NONE: the switch turns ~1.6 MB of preimages into the
    transaction itself and a record per check."""
    import random
    rng = random.Random(7)
    tx = M.rand_tx(rng, 200, (25, 25), [107] * 200)
    code = M.op_script(rng, 25)
    checks = [(tx, code, k, 2, 0, 0) for k in range(200)]
    exp = [M.sighash(*c) for c in checks]
    got_on, kinds_on, _ = H.host_sighash(checks, True)
    got_off, kinds_off, _ = H.host_sighash(checks, False)
    assert got_on == exp and got_off == exp
    assert kinds_on["legacy_rawtx"] == 200 and kinds_off["host_preimage"] == 200


# ------------------------------------------------------------------------------------------------
# the whole engine: the signed fixture with every round on the product's host path


def spends():
    """(items as dicts, flags, (spk, amount, tx, nin) tuples); items of one transaction are adjacent
    and share its bytes, a mutated item has its own copy."""
    d = json.load(gzip.open(os.path.join(GOLDEN, "hashtype_spends.json.gz")))
    txs = [bytes.fromhex(t) for t in d["txs"]]
    tuples = [(bytes.fromhex(it["spk"]), it["amount"], txs[it["tx"]], it["nin"]) for it in d["items"]]
    return d["items"], d["flags"], tuples


def run_stub_batch(E, tuples, flags):
    import bitcoinconsensus_amd as B
    arr, keep = B._batch_items(tuples)
    n = len(tuples)
    ret = (ctypes.c_int * n)()
    err = (ctypes.c_int * n)()
    E.bitcoinconsensus_verify_batch.argtypes = [ctypes.POINTER(B.BatchItem), ctypes.c_size_t,
                                                ctypes.c_uint, ctypes.POINTER(ctypes.c_int),
                                                ctypes.POINTER(ctypes.c_int)]
    rc = E.bitcoinconsensus_verify_batch(arr, n, flags, ret, err)
    assert rc >= 0, rc
    return [(ret[i], err[i]) for i in range(n)]


def test_fixture_holds_what_it_should():
    items, _, _ = spends()
    assert 200 <= len(items) <= 1000
    assert {it["kind"] for it in items} >= {"p2pkh", "p2sh_multisig", "p2wpkh", "p2wsh"}
    assert {it["hashtype"] for it in items} >= {h & 0xff for h, _ in H.BASE_TYPES} | {1}
    assert {it["mutation"] for it in items} >= {"", "hashtype_byte", "output", "other_sequence"}
    mutated = sum(1 for it in items if it["mutation"])
    assert 0.05 * len(items) <= mutated <= 0.2 * len(items)
    nins = {it["tx_inputs"] for it in items}
    assert min(nins) == 1 and max(nins) == 40
    assert any(it["ret"] == 0 for it in items) and any(it["ret"] == 1 for it in items)


@pytest.mark.parametrize("threads", [1, 4])
def test_engine_host_rounds_match_the_reference(threads):
    E, _ = H.host_lib()
    items, flags, tuples = spends()
    exp = [(it["ret"], it["err"]) for it in items]
    E.bcc_set_host_small_round.argtypes = [ctypes.c_size_t]
    E.bcc_set_host_threads.argtypes = [ctypes.c_uint]
    E.bcc_set_host_small_round(1 << 20)  # every round on host_verify_parts, none on the stub stage
    E.bcc_set_host_threads(threads)
    try:
        E.bcc_set_device_hashtypes(1)
        on = run_stub_batch(E, tuples, flags)
        k = H.Kinds()
        E.bcc_last_sighash_kinds(ctypes.byref(k))
        E.bcc_set_device_hashtypes(0)
        off = run_stub_batch(E, tuples, flags)
    finally:
        E.bcc_set_device_hashtypes(0)
        E.bcc_set_host_threads(0)
        E.bcc_set_host_small_round(int(os.environ["BCC_HOST_SMALL_ROUND"]))  # conftest.py's
    bad = [(i, items[i]["kind"], hex(items[i]["hashtype"]), items[i]["mutation"], on[i], exp[i])
           for i in range(len(items)) if on[i] != exp[i]]
    assert not bad, bad[:10]
    assert on == off
    assert k.legacy_rawtx > 0 and k.bip143_rawtx_single > 0 and k.host_preimage == 0
