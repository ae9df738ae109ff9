"""CPU: the sighash model (sighash_model.py) pinned against the reference, the coverage conditions
of the byte-geometry sweeps, and the sweeps through the engine's host twin (job builder + host
lane code over the oracle stub).  test_sighash_geometry_gpu.py runs the same sweeps through the
HIP kernels.

The coverage conditions are asserted on the geometry records alone (formulas of pipeline.h /
engine.cpp over the builders' inputs).  One condition is narrower than "every pos mod 64 from the
IV": a template starts from the IV only while it has fewer than TPL_MID_MIN_BLOCKS blocks
(tpl_len < 436), and pos = 41 (k + 1) for fewer than 253 inputs, so only the ten positions
41, 82, ..., 410 exist without midstates.  The sweep has all ten; all 64 residues are asserted on
the midstate jobs.

The reference takes a one-byte hash type through CheckECDSASignature (ref_check_sighash), so the
sweep checks whose type is wider (0x7fffff01, the negative one, the random 32-bit one) are compared
with the reference under their low byte only by way of the model: the model's handling of 32-bit
types is pinned by the 500 rows of sighash_legacy.json, whose types are random 32-bit values.
The reference accepted every shape of the sweeps (no outputs, 253 inputs, BIP144 form without
outputs): none had to be dropped.
"""
import ctypes
import gzip
import json
import os
import random

import pytest

import sighash_model as M
from oracle_ctypes import Reference, reference_available
from test_sighash_goldens import legacy_checks, random_checks, stub_sighash

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAMILIES = list(M.ECDSA_FAMILIES)
R64 = set(range(64))


def geoms(name):
    return M.family(name)[1]


# ------------------------------------------------------------------------------------------------
# the model against the reference


@pytest.mark.parametrize("which", ["legacy", "random"])
def test_model_matches_committed_reference_sighashes(which):
    checks, exp = legacy_checks() if which == "legacy" else random_checks()
    assert len(checks) == (500 if which == "legacy" else 1200)
    bad = [i for i, c in enumerate(checks) if M.sighash(*c).hex() != exp[i]]
    assert not bad, bad[:10]


def test_model_matches_committed_reference_tapsighashes():
    d = json.load(gzip.open(os.path.join(GOLDEN, "taproot_checks.json.gz")))
    n = 0
    for i, c in enumerate(d["cases"]):
        if c["sighash"] is None:
            continue
        sig = bytes.fromhex(c["sig"])
        got = M.tapsighash(bytes.fromhex(d["blobs"][c["tx"]]), bytes.fromhex(d["blobs"][c["spent"]]),
                           c["nin"], sig[64] if len(sig) == 65 else 0, c["sigversion"],
                           None if c["annex"] is None else bytes.fromhex(c["annex"]),
                           bytes.fromhex(c["tapleaf"]), c["codesep"])
        assert got is not None and got.hex() == c["sighash"], (i, c["cls"])
        n += 1
    assert n >= 1000


@pytest.mark.skipif(not reference_available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("name", FAMILIES)
def test_model_matches_reference_on_ecdsa_sweep(name):
    """Every sweep check through the reference's SignatureHash (hash types of one byte: see the
    module docstring)."""
    R = Reference()
    R.L.ref_check_sighash.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint,
                                      ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint,
                                      ctypes.c_int64, ctypes.c_int, ctypes.c_char_p]
    checks, gs, exp = M.family(name)
    h = ctypes.create_string_buffer(32)
    bad, seen = [], 0
    for i, (tx, code, k, ht, amount, sv) in enumerate(checks):
        low = ht & 0xff
        want = exp[i] if ht == low else M.sighash(tx, code, k, low, amount, sv)
        assert R.L.ref_check_sighash(tx, len(tx), k, code, len(code), low, amount, sv, h) == 1, \
            (name, i, gs[i])
        seen += 1
        if h.raw != want:
            bad.append((i, gs[i]))
    assert not bad, bad[:10]
    assert seen == len(checks)


@pytest.mark.skipif(not reference_available(), reason="oracle/_ref not built")
def test_model_matches_reference_on_taproot_sweep():
    R = Reference()
    checks, gs, exp = M.family("taproot")
    bad = []
    for i, c in enumerate(checks):
        ret, serr, h = R.taproot_check(c["tx"], c["spent"], c["nin"], c["sig"], c["pk"],
                                       c["sigversion"], c["annex"], c["tapleaf"], c["codesep"])
        # a dummy signature: the checker computes the sighash and then fails the BIP340 check
        if ret != 0 or h is None or h != exp[i]:
            bad.append((i, ret, serr, gs[i]))
    assert not bad, bad[:10]


def test_recorded_preimage_lengths_are_the_models():
    """The records' length formulas against the model's own preimages (not the library's)."""
    for name in FAMILIES:
        checks, gs, _ = M.family(name)
        for (tx, code, k, ht, amount, sv), g in zip(checks, gs):
            t = M.parse_tx(tx)
            if g["kind"] == "tpl":
                assert len(M.legacy_preimage(t, code, k, ht)) == g["L"], g
                assert M.script_code_field(code) == M.cs(len(code)) + code
            elif g["kind"] == "legacy_host":
                if not g["single_bug"]:
                    assert len(M.legacy_preimage(t, code, k, ht)) == g["pre_len"], g
            else:
                assert len(M.bip143_preimage(t, code, k, ht, amount)) == g["pre_len"], g
                if g["kind"] == "wtx":
                    assert len(t["vin"]) == g["nin"] and sum(map(len, t["vout"])) == g["outs_len"]


# ------------------------------------------------------------------------------------------------
# coverage conditions (on the geometry records alone)


def test_sweep_size():
    total = sum(len(M.family(n)[0]) for n in FAMILIES + ["taproot"])
    assert 5000 <= total <= 40000, total


def test_coverage_legacy_all_templates():
    gs = geoms("legacy_all")
    assert all(g["kind"] == "tpl" and M.legacy_all_type(g["ht"]) for g in gs)
    iv = [g for g in gs if not g["mid"]]
    mid = [g for g in gs if g["mid"]]
    # splice position: every residue from a midstate; from the IV every position that exists
    # (module docstring)
    assert {g["pos"] % 64 for g in mid} == R64
    assert {g["pos"] for g in iv} >= {41 * (k + 1) for k in range(10)}
    assert all(g["tpl_len"] < 436 for g in iv) and all(g["tpl_len"] >= 436 for g in mid)
    for part in (iv, mid):
        assert {(g["pos"] % 4, g["cl"] % 4) for g in part} == {(a, b) for a in range(4) for b in range(4)}
        assert {g["L"] % 64 for g in part} == R64
        for r in list(range(51, 64)) + [0]:
            assert len({g["pos"] % 4 for g in part if g["L"] % 64 == r}) == 4, r
        cls = {g["cl"] for g in part}
        assert cls >= set(range(1, 142))                                  # 1 = an empty scriptCode
        assert {g["code_len"] for g in part} >= set(range(253, 263))      # 3-byte compact size
        # the code field inside one block, across one boundary, over three blocks
        spans = {(g["pos"] + g["cl"] - 1) // 64 - g["pos"] // 64 for g in part if g["cl"] > 0}
        assert spans >= {0, 1, 2}
        # splice in a fast block, in the last fast block, in the trailer; code ending in the trailer
        assert any(g["fast"] >= 2 and g["pos"] // 64 < g["fast"] - 1 for g in part)
        assert any(g["fast"] >= 1 and g["pos"] // 64 == g["fast"] - 1 for g in part)
        assert any(g["pos"] >= 64 * g["fast"] for g in part)
        assert any(g["pos"] < 64 * g["fast"] < g["pos"] + g["cl"] for g in part)
    # the smallest messages: one block (L = 55) and two (L = 56), no fast block
    assert any(g["fast"] == 0 and g["L"] == 55 and g["nblk"] == 1 and g["cl"] == 1 for g in iv)
    assert any(g["fast"] == 0 and g["L"] == 56 and g["nblk"] == 2 and g["cl"] == 2 for g in iv)
    # midstate jobs that start at block 0 and that start at the trailer
    assert any(g["pos"] // 64 == 0 for g in mid)
    assert any(g["pos"] // 64 == g["fast"] for g in mid)
    assert {252, 253} <= {g["nin"] for g in mid}
    # hash types: the five of the issue, and no trailer byte position that is always zero
    hts = {g["ht"] for g in gs}
    assert hts == {h & 0xffffffff for h in M.tpl_hashtypes()} and len(hts) == 5
    assert {0x01, 0x41, 0x7fffff01, 0x80000001} < hts
    for s in (0, 8, 16, 24):
        assert any((h >> s) & 0xff for h in hts)
    # every hash type at the 55/56-byte edge and on both start kinds
    for h in hts:
        assert {g["L"] for g in iv if g["ht"] == h} >= {55, 56}
        assert any(g["ht"] == h for g in mid)


def test_coverage_legacy_tx_order():
    gs = geoms("legacy_tx_order")
    # whole transactions, inputs in order; one of them across the 253-input count field
    runs, k = [], None
    for g in gs:
        if g["k"] == 0:
            runs.append(0)
        assert g["k"] == runs[-1]
        runs[-1] += 1
    assert runs == [7, 70, 70, 253]
    assert any(g["mid"] for g in gs) and any(not g["mid"] for g in gs)


def test_coverage_legacy_other_types():
    gs = geoms("legacy_other")
    assert {g["ht"] for g in gs} == {2, 3, 0x82, 0x83, 0x81}
    for ht in (2, 3, 0x82, 0x83):
        assert {g["pre_len"] % 64 for g in gs if g["ht"] == ht and not g["single_bug"]} == R64, ht
    assert sum(g["single_bug"] for g in gs) >= 20
    assert {g["ht"] for g in gs if g["single_bug"]} == {3, 0x83}


def test_coverage_bip143_rawtx():
    gs = geoms("bip143")
    assert {g["nin"] for g in gs} >= set(M.NIN_LIST)
    assert set(M.NIN_LIST) >= set(range(1, 41)) | {63, 64, 65, 113, 114, 252, 253}
    assert {g["seq_len"] % 64 for g in gs} == set(range(0, 64, 4))
    assert {g["prevouts_len"] % 64 for g in gs} == set(range(0, 64, 4))
    assert {56, 60} <= {g["seq_len"] % 64 for g in gs}  # hashSequence's extra padding block
    for nin in M.NIN_LIST:  # both wire forms
        assert {g["witness"] for g in gs if g["nin"] == nin} == {False, True}, nin
    assert any(g["wtx3"] for g in gs) and any(g["witness"] and not g["wtx3"] for g in gs)
    for form in (False, True):
        part = [g for g in gs if g["wtx3"] == form]
        assert any(g["nout"] == 0 for g in gs if g["witness"] == form)
        assert {g["outs_len"] % 64 for g in part if g["nout"]} == R64
        assert {a for g in part for a in g["outpoint_align"]} == {0, 1, 2, 3}
    assert {a % 128 for g in gs for a in g["cs3_at"]} == set(range(128))
    assert {g["pre_len"] % 64 for g in gs} == R64
    assert {g["code_len"] for g in gs} >= {251, 252, 253, 254}
    assert {g["ht"] for g in gs} == {1, 2, 0x81, 0x82}
    for ht in (1, 2, 0x81, 0x82):
        assert {g["pre_len"] % 64 for g in gs if g["ht"] == ht} == R64


def test_coverage_bip143_single():
    gs = geoms("bip143_single")
    assert {g["code_len"] for g in gs} == set(range(71))
    assert {g["slot"] % 16 for g in gs} == set(range(16))
    for ht in (3, 0x83):
        for has in (False, True):
            assert {g["slot"] % 4 for g in gs if g["ht"] == ht and g["has_output"] == has} == {0, 1, 2, 3}


def test_coverage_taproot():
    gs = geoms("taproot")
    assert {g["nin"] for g in gs} >= set(M.NIN_LIST)
    assert {g["spent_len"] for g in gs} >= set(M.SPENT_LENS)
    assert set(M.SPENT_LENS) == set(range(141)) | set(range(253, 261))
    acp = [g for g in gs if g["ht"] & 0x80]
    assert {g["spent_len"] for g in acp} >= set(M.SPENT_LENS)
    assert any(g["nout"] == 0 for g in gs)
    assert {g["outs_len"] % 64 for g in gs if g["nout"]} == R64
    assert {g["ht"] for g in gs} == set(M.TAP_HASHTYPES)
    assert all(g["ht"] & 3 != 3 or g["k"] < g["nout"] for g in gs)
    for sv in (0, 1):
        part = [g for g in gs if g["sigversion"] == sv]
        assert {g["ht"] for g in part} == set(M.TAP_HASHTYPES)
        assert {g["annex_len"] for g in part} >= set(range(121)) | {None}
    ts = [g for g in gs if g["sigversion"] == 1]
    assert 0xFFFFFFFF in {g["codesep"] for g in ts} and {0, 1, 2, 3} <= {g["codesep"] for g in ts}


# ------------------------------------------------------------------------------------------------
# the host twin: the engine's job builder and host lane code over the oracle stub


@pytest.mark.parametrize("name", FAMILIES)
def test_host_twin_matches_model_on_ecdsa_sweep(name):
    checks, _, _ = M.family(name)
    msg = M.mismatches(name, stub_sighash(checks))
    assert not msg, msg


def test_host_twin_matches_model_all_families_shuffled():
    checks, exp, gs = [], [], []
    for name in FAMILIES:
        c, g, e = M.family(name)
        checks += c
        exp += e
        gs += [dict(x, family=name) for x in g]
    order = list(range(len(checks)))
    random.Random(M.SEED).shuffle(order)
    got = stub_sighash([checks[i] for i in order])
    msg = M.mismatches("all families, shuffled", got, [exp[i] for i in order], [gs[i] for i in order])
    assert not msg, msg


def test_host_twin_matches_model_on_taproot_sweep():
    import bitcoinconsensus_amd as B
    import engine_stub
    checks, _, _ = M.family("taproot")
    out, hs = B.taproot_verify_batch(checks, sighashes=True, library=engine_stub.load())
    assert all(r != -1 for r, _ in out), [i for i, (r, _) in enumerate(out) if r == -1][:10]
    msg = M.mismatches("taproot", hs)
    assert not msg, msg
