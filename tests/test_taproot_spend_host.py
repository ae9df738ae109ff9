"""CPU: bcc_taproot_spend_batch's host code (csrc/host/taproot_spend.cpp: the witness rules, the
tapscript interpreter of csrc/host/script.cpp with the deferring checker, the commitment lane code
of csrc/taproot_commit.h on the host, the round cut, parts and device sharding) in the device-less
engine build (tests/engine_stub.py), against every committed case of
tests/golden/taproot_spends.json.gz.

Class r_* cases carry the reference's VerifyScript answer.  For class s_* cases (signatures) NO
reference whole-spend verdict exists: the oracle's VerifyScript asserts on any Schnorr check, so
the expectation is the entry point's documented rule applied to the reference's per-check answers
(CheckSchnorrSignature through ref_taproot_check): the first non-empty signature in execution order
whose check fails gives (0, its serror), else the template's arithmetic (taproot_spend_cases).
The -m gpu twin (test_taproot_spend_gpu.py) runs the same cases through librbc_amd.so."""
import ctypes
import random

import pytest

import bitcoinconsensus_amd as B
import engine_stub
import taproot_spend_cases as S
from oracle_ctypes import Reference, reference_available


@pytest.fixture(scope="module")
def L():
    return engine_stub.load()


@pytest.fixture(scope="module")
def golden():
    return S.load_golden()


def check_cases(out, cases):
    bad = [(i, c["cls"], tuple(o), c["expected"]) for i, (o, c) in enumerate(zip(out, cases))
           if tuple(o) != tuple(c["expected"])]
    assert len(out) == len(cases) and not bad, bad[:10]


def test_spend_golden_cases_on_host(L, golden):
    check_cases(B.taproot_spend_batch(S.items_of(golden), library=L), golden)


def test_spend_golden_covers_what_it_should(golden):
    errs = {c["expected"][1] for c in golden}
    assert S.LISTED_ERRORS <= errs, S.LISTED_ERRORS - errs
    assert {c["cls"][:2] for c in golden} == {"r_", "s_"}
    valid = sum(c["expected"] == (1, 0) for c in golden)
    assert 0.3 * len(golden) <= valid <= 0.7 * len(golden)


def test_spend_single_items_equal_the_batch(L, golden):
    for c in golden[::7]:
        assert B.taproot_spend_batch(S.items_of([c]), library=L) == [tuple(c["expected"])], c["cls"]


def test_spend_checks_agree_piece_by_piece(L, golden):
    """Every queued check through bcc_taproot_verify_batch with the codesep_pos the test computed
    and the leaf hash of the spend's script: the verdict the reference recorded for that check."""
    checks, want = [], []
    for c in golden:
        for k in c.get("checks", []):
            checks.append(dict(tx=c["tx"], spent=c["spent"], nin=c["nin"], sig=k["sig"], pk=k["pk"],
                               sigversion=B.SIGVERSION_TAPROOT if k["leaf"] is None else B.SIGVERSION_TAPSCRIPT,
                               annex=k["annex"], tapleaf=k["leaf"], codesep=k["codesep"]))
            want.append(k["ref"])
    assert len(checks) > 100
    got = B.taproot_verify_batch(checks, library=L)
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if tuple(g) != tuple(w)]
    assert not bad, bad[:10]


def test_spend_parts_rounds_and_sharding(L, golden):
    """More than two host parts (> 2 x 1024 items), a round boundary inside the batch (and inside a
    run of one tx's inputs), and the device list [0, 1, 2]: all equal to the one-device answer."""
    small = [c for c in golden if len(c["tx"]) < 600]
    rng = random.Random(5)
    cases = [rng.choice(small) for _ in range(2300)]
    multi = [c for c in golden if c["cls"].startswith("s_multi_input")][:4]
    assert len({id(c["tx"]) for c in multi}) == 1
    cases[998:998] = multi  # items 998 .. 1001: one tx across the cut at 1000
    items = S.items_of(cases)
    out = B.taproot_spend_batch(items, library=L)
    check_cases(out, cases)
    try:
        B.set_spend_round(1000, library=L)
        assert B.taproot_spend_batch(items, library=L) == out
        B.set_spend_round(1, library=L)
        assert B.taproot_spend_batch(items[:300], library=L) == out[:300]
    finally:
        B.set_spend_round(0, library=L)
    try:
        engine_stub.set_devices(L, [0, 1, 2])
        big = items * 3  # > 4096 items: the batch is really spread
        out3 = B.taproot_spend_batch(big, device=-1, library=L)
    finally:
        engine_stub.set_devices(L, [])
    assert out3 == out * 3


def test_spend_null_and_empty(L, golden):
    assert B.taproot_spend_batch([], library=L) == []
    fn = L.bcc_taproot_spend_batch
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    one = (B.TaprootSpend * 1)()
    ret, err = (ctypes.c_int * 1)(7), (ctypes.c_int * 1)(7)
    assert fn(None, 0, None, None, 0) == 0
    assert fn(None, 1, ret, err, 0) == -1
    assert fn(one, 1, None, err, 0) == -1 and fn(one, 1, ret, None, 0) == -1
    assert fn(one, 1, ret, err, 0) == -1  # null tx / spent_outputs
    c = golden[0]
    one[0] = B.TaprootSpend(c["tx"], len(c["tx"]), None, 0, c["nin"])
    assert fn(one, 1, ret, err, 0) == -1
    assert (ret[0], err[0]) == (7, 7)  # nothing was verified


def test_spend_refused_inputs(L, golden):
    """ret -1 / serror 1: a tx with trailing bytes, a spent-output count that differs, an input index
    out of range, and a spent scriptPubKey that is no native v1 program."""
    c = next(c for c in golden if c["cls"] == "s_keypath_00")
    it = S.items_of([c])[0]
    n_in = c["spent"][0]
    p2wpkh = c["spent"][:1] + (c["spent"][1:9] + b"\x16\x00\x14" + bytes(20)) * n_in
    v0_32 = c["spent"][:1] + (c["spent"][1:9] + b"\x22\x00\x20" + bytes(32)) * n_in
    v1_31 = c["spent"][:1] + (c["spent"][1:9] + b"\x21\x51\x1f" + bytes(31)) * n_in
    bad = [dict(it, tx=it["tx"] + b"\x00"), dict(it, tx=it["tx"][:-1]), dict(it, spent=it["spent"] + b"\x00"),
           dict(it, spent=b"\x00"), dict(it, nin=n_in), dict(it, spent=p2wpkh), dict(it, spent=v0_32),
           dict(it, spent=v1_31)]
    assert B.taproot_spend_batch([it] + bad, library=L) == [(1, 0)] + [(-1, 1)] * len(bad)


def test_spend_scriptsig_that_depends_on_an_ecdsa_verdict_is_refused(L, golden):
    """A non-empty scriptSig is decided where no ECDSA verdict matters (the golden r_scriptsig_*
    cases); where the result depends on one (CHECKSIGVERIFY) or more than one check is met, the
    entry says ret -1 / serror 1, as its header documents."""
    import random as _r
    rng = _r.Random(3)
    prog, wit, _ = S.script_path(rng, S.OP_1, [])
    key = S.push(bytes([2]) * 33)
    items = []
    for ss in (S.push(S.DER_SIG) + key + S.OP_CHECKSIGVERIFY,
               (S.push(S.DER_SIG) + key + S.OP_CHECKSIG) * 2):
        t = S.G.make_tx(rng, nin=1, nout=1, long_ok=False)
        S.place(rng, t, 0, prog, wit, script_sig=ss)
        items.append(dict(tx=S.G.tx_bytes(t), spent=S.G.ser_outs(t["spent"]), nin=0))
    assert B.taproot_spend_batch(items, library=L) == [(-1, 1), (-1, 1)]


def test_verify_script_is_unchanged_for_v1_and_checksigadd(L, golden):
    """bitcoinconsensus_verify_* behaves as before: v1 programs pass unchecked there
    (SCRIPT_VERIFY_TAPROOT is not a libconsensus flag, and a flag set that names it is refused), and
    OP_CHECKSIGADD stays BAD_OPCODE outside tapscript (here in a P2WSH script, so nothing passes)."""
    import hashlib
    from test_host_engine import call
    c = next(c for c in golden if c["cls"] == "r_checkmultisig")
    assert c["expected"] == (0, 49)
    spk = S._spent_script(c["spent"], c["nin"])
    assert call(L, spk, 0, c["tx"], c["nin"], 0xE15) == (1, 0)
    assert call(L, spk, 0, c["tx"], c["nin"], 0xE15 | 1 << 17) == (0, 5)  # ERR_INVALID_FLAGS
    script = b"\x00\x00\x00\xba"
    tx = S.G.ser_tx(2, [(bytes(36), b"", 0)], [(0, b"\x51")], 0, [[script]])
    assert call(L, b"\x00\x20" + hashlib.sha256(script).digest(), 0, tx, 0, 0xE15) == (0, 0)


@pytest.mark.skipif(not reference_available(), reason="needs the reference build (oracle/_ref)")
def test_random_mix_against_the_reference_alone():
    """The random generator the GPU test draws from: between 30 % and 70 % of its spends verify and
    every listed error code occurs, by the reference's answers alone."""
    cases = S.random_cases(Reference(), random.Random(0xA11CE), 400)
    valid = sum(c["expected"] == (1, 0) for c in cases)
    assert 0.3 * len(cases) <= valid <= 0.7 * len(cases), valid
    errs = {c["expected"][1] for c in cases}
    assert S.LISTED_ERRORS <= errs, S.LISTED_ERRORS - errs


@pytest.mark.skipif(not reference_available(), reason="needs the reference build (oracle/_ref)")
def test_spend_random_cases_on_host(L):
    cases = S.random_cases(Reference(), random.Random(0xB0B), 300)
    check_cases(B.taproot_spend_batch(S.items_of(cases), library=L), cases)
