"""GPU: the Taproot side's host path against the device through librbc_amd.so: the same checks on
the kernels and on the host evaluation (csrc/host/taproot_host.cpp), the default small-round
threshold, and the injected-fault sequence of test_taproot_hostpath.py against the real device
seams.  An injected fault fails a round before it is launched, so nothing here makes the GPU
fail."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bitcoinconsensus_amd as B
import taproot_hostpath_cases as H
import taproot_spend_cases as S
from fixtures import bip340_vectors, schnorr_exceptional, taproot_checks
from test_taproot_hostpath import check_against_golden

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(HERE, "..", "rust-bitcoinconsensus_amd")


def test_taproot_checks_host_against_device():
    cases = taproot_checks()
    dev = B.taproot_verify_batch(cases, sighashes=True)
    st_dev = B.last_taproot_stats()
    with H.settings(None, small_round=H.HOST_ALL):
        host = B.taproot_verify_batch(cases, sighashes=True)
        st_host = B.last_taproot_stats()
    assert host == dev
    check_against_golden(dev[0], dev[1], cases)
    assert st_dev["host_rounds"] == 0 and st_dev["rounds"] >= 1 and st_dev["host_checks"] == 0
    assert st_host["host_rounds"] == st_host["rounds"] >= 1
    assert st_host["checks"] == st_dev["checks"] == st_host["host_checks"] > 1000


def test_bip340_tuples_host_against_device():
    n = 20_000
    vec = [(t["sig"], t["msg"], t["pub"], t["verdict"]) for t in bip340_vectors() + schnorr_exceptional()]
    ts = B.TupleSet(n, kind="c5", seed=0x7A9007, vectors=vec)
    try:
        ts.run()
        gpu = np.frombuffer(ts.verdicts(), np.uint8)
        h = ts.host()
        sig, msg, pub = (h[k].tobytes() for k in ("sig64", "msg32", "xonly32"))
        want = np.array(h["expect"], np.uint8)
    finally:
        ts.free()
    host = np.frombuffer(B.host_schnorr_verify_tuples(sig, msg, pub, threads=16), np.uint8)
    assert 0 < int(want.sum()) < n
    assert np.array_equal(gpu, want), np.nonzero(gpu != want)[0][:20]
    assert np.array_equal(host, want), np.nonzero(host != want)[0][:20]
    # the entry point on both paths over a slice of the same rows
    k = 600
    dev = B.schnorr_verify_tuples(sig[:64 * k], msg[:32 * k], pub[:32 * k])
    assert B.last_taproot_stats()["host_rounds"] == 0
    with H.settings(None, small_round=H.HOST_ALL):
        small = B.schnorr_verify_tuples(sig[:64 * k], msg[:32 * k], pub[:32 * k])
        st = B.last_taproot_stats()
    assert dev == small == want[:k].tobytes()
    assert (st["rounds"], st["host_rounds"], st["host_checks"]) == (1, 1, k)


def test_default_threshold_sends_a_lone_input_to_the_host_and_a_batch_to_the_device():
    gold = S.load_golden()
    lone = [next(c for c in gold if c["cls"].startswith("s_keypath") and tuple(c["expected"]) == (1, 0)),
            next(c for c in gold if any(k["leaf"] is not None for k in c.get("checks", []))
                 and tuple(c["expected"]) == (1, 0)),
            next(c for c in gold if c.get("checks") and tuple(c["expected"]) == (0, 46))]
    keypath = [c for c in taproot_checks() if c["sigversion"] == B.SIGVERSION_TAPROOT
               and c["ret"] != -1 and c["serror"] in (0, B.SCRIPT_ERR_SCHNORR_SIG)][:64]
    assert len(keypath) == 64 and {c["ret"] for c in keypath} == {0, 1}
    with H.settings(None, small_round=B.HOST_SMALL_ROUND_DEFAULT):
        for c in lone:
            assert B.verify_input(c["tx"], c["spent"], c["nin"]) == (c["expected"][0], 0), c["cls"]
            st = B.last_taproot_stats()
            assert st["host_rounds"] == st["rounds"] == 1, (c["cls"], st)
        out = B.taproot_verify_batch(keypath)
        st = B.last_taproot_stats()
    assert out == [(c["ret"], c["serror"]) for c in keypath]
    assert (st["checks"], st["rounds"], st["host_rounds"]) == (64, 1, 0)


_FAULTS_CHILD = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import bitcoinconsensus_amd as B
import taproot_hostpath_cases as H
from fixtures import taproot_checks
assert H.fault_sequence(None)
# bcc_taproot_verify_batch's pipelined rounds (BCC_TAPROOT_ROUND=64, read at load): a round that
# fails at its launch is rebuilt from its items while later rounds are built and launched
cases = taproot_checks()[:1500]
want = B.taproot_verify_batch(cases, sighashes=True)
st = B.last_taproot_stats()
assert st["rounds"] >= 8 and st["host_rounds"] == 0, st
L = H.bind(None)
for inject, allowed in ((lambda: L.bcc_debug_fail_device_rounds(1), (1, 0)),
                        (lambda: L.bcc_debug_fail_device_rounds(2), (1, 1)),
                        (lambda: L.bcc_debug_fail_device_rounds_code(1, 719), (0, 1)),
                        (lambda: L.bcc_debug_fail_device_rounds_code(1 << 20, 719), (0, st["rounds"]))):
    inject()
    try:
        got = B.taproot_verify_batch(cases, sighashes=True)
    finally:
        L.bcc_debug_fail_device_rounds(0)
    t = B.last_taproot_stats()
    assert got == want and (t["device_retries"], t["host_rounds"]) == allowed, t
    assert t["rounds"] == st["rounds"] and t["checks"] == st["checks"]
# the entries whose rounds live beside the kernels: commitments, tweak tuples, BIP340 tuples
import commit_cases as C
spends, tuples = C.load_golden()
rows = C.tuple_rows([(t["cls"], t["q"], t["parity"], t["p"], t["t"]) for t in tuples])
sig = [(c["sig"][:64], c["sighash"], c["pk"]) for c in cases if c["sighash"] is not None
       and len(c["sig"]) in (64, 65)]
sig = [b"".join(r[k] for r in sig) for k in range(3)]
calls = dict(commit=lambda: B.taproot_commit_batch(spends, tapleaf=True),
             tweak=lambda: B.xonly_tweak_check_tuples(*rows),
             schnorr=lambda: B.schnorr_verify_tuples(*sig))
for name, call in calls.items():
    want = call()
    base = B.last_taproot_stats()
    assert (base["rounds"], base["host_rounds"], base["device_retries"]) == (1, 0, 0), (name, base)
    for inject, allowed in ((lambda: L.bcc_debug_fail_device_rounds(1), (1, 0)),
                            (lambda: L.bcc_debug_fail_device_rounds(2), (1, 1)),
                            (lambda: L.bcc_debug_fail_device_rounds_code(1, 719), (0, 1))):
        before = B.host_fallback_rounds()
        inject()
        try:
            got = call()
        finally:
            L.bcc_debug_fail_device_rounds(0)
        t = B.last_taproot_stats()
        assert got == want and (t["device_retries"], t["host_rounds"]) == allowed, (name, t)
        assert t["host_checks"] == allowed[1] * (base["checks"] + base["commits"]), (name, t)
        assert B.host_fallback_rounds() - before == allowed[1], name
    L.bcc_set_device_failure_policy(B.DEVICE_FAILURE_ERROR)
    L.bcc_debug_fail_device_rounds(2)
    try:
        call()
        raise SystemExit(name + ": no error under BCC_DEVICE_FAILURE_ERROR")
    except RuntimeError:
        pass
    finally:
        L.bcc_debug_fail_device_rounds(0)
        L.bcc_set_device_failure_policy(B.DEVICE_FAILURE_HOST)
    assert call() == want, name
print("ok")
"""


def test_injected_faults_against_the_real_device():
    """The fault sequence of the CPU suite on the spend and mixed goldens, then the pipelined
    rounds of bcc_taproot_verify_batch and the commitment, tweak-tuple and BIP340-tuple entries
    under the same faults.  In a child process: the fallback counter is per process and the
    suite's fixture watches it."""
    env = dict(os.environ, BCC_HOST_SMALL_ROUND="0", BCC_TAPROOT_ROUND="64")
    p = subprocess.run([sys.executable, "-c", _FAULTS_CHILD, PKG, HERE], capture_output=True,
                       text=True, timeout=240, env=env)
    assert p.returncode == 0 and "ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-3000:])


_SPARSE_CHILD = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import bitcoinconsensus_amd as B
from fixtures import taproot_checks
from test_taproot_hostpath import check_against_golden
cases = taproot_checks()
reach = [c for c in cases if c["ret"] != -1 and c["serror"] in (0, 46)]
early = [c for c in cases if c["ret"] == 0 and c["serror"] in (44, 45)]
early = (early * (64 // len(early) + 1))[:64]
assert len(reach) >= 400 and len(early) == 64

def own_tx(cs):  # every check its own tx buffer: a round is then cut at exactly 64 items
    return [dict(c, tx=bytes(bytearray(c["tx"])), spent=bytes(bytearray(c["spent"]))) for c in cs]

B.set_host_small_round(B.HOST_SMALL_ROUND_DEFAULT)
for name, middle, host_rounds in (("few rows", early[:56] + reach[300:308], 1),
                                  ("no rows", early, 0)):
    # rounds 0 and 1 are in flight when the middle round launches nothing; three more follow
    batch = own_tx(reach[:128] + middle + reach[128:320])
    out, hs = B.taproot_verify_batch(batch, sighashes=True)
    check_against_golden(out, hs, batch)
    st = B.last_taproot_stats()
    assert st["rounds"] == 5 + host_rounds and st["host_rounds"] == host_rounds, (name, st)
    assert st["checks"] == 320 + 8 * host_rounds and st["host_checks"] == 8 * host_rounds, (name, st)
B.set_host_small_round(0)
batch = own_tx(reach[:128] + early[:56] + reach[300:308] + reach[128:320])
out, hs = B.taproot_verify_batch(batch, sighashes=True)
check_against_golden(out, hs, batch)
st = B.last_taproot_stats()
assert (st["rounds"], st["host_rounds"]) == (6, 0), st
assert B.host_fallback_rounds() == 0
print("ok")
"""


def test_pipelined_rounds_with_a_middle_round_that_launches_nothing():
    """bcc_taproot_verify_batch in 64-check pipelined rounds (BCC_TAPROOT_ROUND, read at load: a
    child process) at the default threshold: a middle round in which only 8 checks reach BIP340
    runs on the host, and one in which none does launches nothing, while two earlier rounds are in
    flight.  The slot rotation must not hand a later round the slot of a round still in flight:
    every item equals the golden value, sighash included."""
    env = dict(os.environ, BCC_TAPROOT_ROUND="64")
    p = subprocess.run([sys.executable, "-c", _SPARSE_CHILD, PKG, HERE], capture_output=True,
                       text=True, timeout=120, env=env)
    assert p.returncode == 0 and "ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-3000:])
