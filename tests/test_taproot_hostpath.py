"""CPU: the Taproot side's host path (csrc/host/taproot_host.cpp) and its failure handling, in the
device-less engine build (tests/engine_stub.py) unless stated.

With the small-round threshold above every batch the engine's own verdict code runs: host SHA-256
over the job records the kernels read and the kernels' BIP340 lane over the host comb
(host_taproot_parts), where the stub device otherwise answers with the oracle.  With the threshold
at 0 the stub device answers, and injected faults drive the retry, the failure policy and the
rebuild of a failed round.  Expected values are the reference's, from tests/golden/.
The -m gpu twin (test_taproot_hostpath_gpu.py) runs the same through librbc_amd.so."""
import ctypes
import os
import subprocess
import sys

import pytest

import bitcoinconsensus_amd as B
import engine_stub
import mixed_input_cases as M
import taproot_hostpath_cases as H
import taproot_spend_cases as S
from fixtures import (bip340_vectors, schnorr_exceptional, schnorr_tuples, structured_scalars,
                      taproot_checks)

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(HERE, "..", "rust-bitcoinconsensus_amd")


@pytest.fixture(scope="module")
def L():
    return H.bind(engine_stub.load())


def check_against_golden(out, hs, cases):
    bad = []
    for i, ((ret, serr), h, c) in enumerate(zip(out, hs, cases)):
        if ret != c["ret"]:
            bad.append((i, c["cls"], "ret", ret, c["ret"]))
        elif ret == 0 and serr != c["serror"]:
            bad.append((i, c["cls"], "serror", serr, c["serror"]))
        elif ret == -1 and serr != 1:
            bad.append((i, c["cls"], "refused serror", serr))
        want = c["sighash"] if c["sighash"] is not None else bytes(32)
        if ret != -1 and h != want:
            bad.append((i, c["cls"], "sighash"))
    assert not bad, bad[:10]


def test_host_schnorr_tuples_match_their_labels(L):
    rows = bip340_vectors() + schnorr_tuples() + schnorr_exceptional() + structured_scalars()["schnorr"]
    assert len(rows) > 500 and {r["verdict"] for r in rows} == {0, 1}
    sig, msg, pub = (b"".join(r[k] for r in rows) for k in ("sig", "msg", "pub"))
    one = B.host_schnorr_verify_tuples(sig, msg, pub, threads=1, library=L)
    bad = [(i, r["cls"], one[i], r["verdict"]) for i, r in enumerate(rows) if one[i] != r["verdict"]]
    assert not bad, bad[:10]
    assert B.host_schnorr_verify_tuples(sig, msg, pub, threads=4, library=L) == one
    assert B.host_schnorr_verify_tuples(b"", b"", b"", library=L) == b""
    f = L.bcc_host_schnorr_verify_tuples
    f.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_uint]
    assert f(None, None, None, None, 0, 1) == 0 and f(None, msg, pub, None, 1, 1) == -1


def test_python_struct_matches_c_layout(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bcc_amd.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(bcc_taproot_stats),'
                   ' offsetof(bcc_taproot_stats, device_retries)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(HERE, "..", "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(B.TaprootStats), B.TaprootStats.device_retries.offset]


def test_taproot_checks_on_the_host_path(L):
    cases = taproot_checks()
    assert len(cases) == 2155
    with H.settings(L, small_round=H.HOST_ALL):
        out, hs = B.taproot_verify_batch(cases, sighashes=True, library=L)
        st = B.last_taproot_stats(library=L)
        check_against_golden(out, hs, cases)
        assert st["items"] == len(cases) and st["commits"] == 0
        assert st["checks"] == sum(c["ret"] != -1 and c["serror"] in (0, B.SCRIPT_ERR_SCHNORR_SIG)
                                   for c in cases)
        assert st["host_rounds"] == st["rounds"] >= 1 and st["host_checks"] == st["checks"]
        assert st["device_retries"] == 0
        first = {}
        for i, c in enumerate(cases):
            first.setdefault(c["cls"], i)
        for i in first.values():
            o, h = B.taproot_verify_batch([cases[i]], sighashes=True, library=L)
            assert (o[0], h[0]) == (out[i], hs[i]), cases[i]["cls"]
    # the stub device (the oracle) on the same cases: the two evaluations agree row by row
    out0, hs0 = B.taproot_verify_batch(cases, sighashes=True, library=L)
    assert (out0, hs0) == (out, hs)
    assert B.last_taproot_stats(library=L)["host_rounds"] == 0


@pytest.mark.parametrize("spend_round", [0, 64])
def test_golden_spends_and_mixed_inputs_on_the_host_path(L, spend_round):
    spends, spends_want = H.spend_golden()
    cases, mixed, mixed_want = H.mixed_golden()
    before = L.bcc_host_fallback_rounds()
    with H.settings(L, small_round=H.HOST_ALL, spend_round=spend_round):
        assert B.taproot_spend_batch(spends, library=L) == spends_want
        st = B.last_taproot_stats(library=L)
        assert st["items"] == len(spends) and st["checks"] > 100 and st["commits"] > 50
        assert st["host_rounds"] == st["rounds"] >= (4 if spend_round else 1)
        assert st["host_checks"] == st["checks"] + st["commits"]
        assert B.verify_inputs_batch(mixed, H.F, library=L) == mixed_want
        st = B.last_taproot_stats(library=L)  # the side thread's call, handed to this thread
        assert st["items"] == sum(c["v1"] for c in cases) > 0
        assert st["host_rounds"] == st["rounds"] >= 1
        assert st["host_checks"] == st["checks"] + st["commits"] > 0
        c = next(c for c in cases if c["v1"] and c["expected"] == (1, 0))
        assert B.verify_input(c["tx"], c["spent"], c["nin"], H.F, library=L) == (1, 0)
        st = B.last_taproot_stats(library=L)
        assert (st["items"], st["rounds"], st["host_rounds"]) == (1, 1, 1)
    assert L.bcc_host_fallback_rounds() == before  # a small round is no fallback


def test_injected_faults_retry_fall_back_and_report(L):
    assert H.fault_sequence(L)


def test_a_failed_round_of_taproot_verify_batch(L):
    """bcc_taproot_verify_batch's own round under the same rules (one round here: its pipelined
    form needs more checks than a CPU test should hash)."""
    cases = taproot_checks()[::5]
    want = B.taproot_verify_batch(cases, sighashes=True, library=L)
    with H.settings(L):
        for inject, retries, host_rounds in ((lambda: L.bcc_debug_fail_device_rounds(1), 1, 0),
                                             (lambda: L.bcc_debug_fail_device_rounds(2), 1, 1),
                                             (lambda: L.bcc_debug_fail_device_rounds_code(1, 719), 0, 1)):
            before = L.bcc_host_fallback_rounds()
            inject()
            assert B.taproot_verify_batch(cases, sighashes=True, library=L) == want
            st = B.last_taproot_stats(library=L)
            assert (st["device_retries"], st["host_rounds"], st["rounds"]) == (retries, host_rounds, 1)
            assert L.bcc_host_fallback_rounds() - before == host_rounds
        L.bcc_set_device_failure_policy(B.DEVICE_FAILURE_ERROR)
        L.bcc_debug_fail_device_rounds(3)
        with pytest.raises(RuntimeError):
            B.taproot_verify_batch(cases, library=L)
        L.bcc_debug_fail_device_rounds(0)
        assert B.taproot_verify_batch(cases, sighashes=True, library=L) == want


_PRODUCT_CHILD = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import bitcoinconsensus_amd as B
import taproot_spend_cases as S
from fixtures import taproot_checks
from test_taproot_hostpath import check_against_golden
cases = taproot_checks()
out, hs = B.taproot_verify_batch(cases, sighashes=True)
check_against_golden(out, hs, cases)
st = B.last_taproot_stats()
assert st["host_rounds"] == st["rounds"] >= 1 and st["host_checks"] == st["checks"] > 1000, st
gold = S.load_golden()
key = next(c for c in gold if c["cls"].startswith("s_keypath") and tuple(c["expected"]) == (1, 0))
script = next(c for c in gold if any(k["leaf"] is not None for k in c.get("checks", []))
              and tuple(c["expected"]) == (1, 0))
bad = next(c for c in gold if c.get("checks") and tuple(c["expected"]) == (0, 46))
for c in (key, script, bad):
    assert B.verify_input(c["tx"], c["spent"], c["nin"]) == (c["expected"][0], 0), c["cls"]
    st = B.last_taproot_stats()
    assert st["host_rounds"] == st["rounds"] == 1 and st["host_checks"] >= 1, (c["cls"], st)
rows = [(c["sig"][:64], c["sighash"], c["pk"], c["ret"]) for c in cases
        if c["sighash"] is not None and len(c["sig"]) in (64, 65) and c["serror"] in (0, 46)]
got = B.schnorr_verify_tuples(*(b"".join(r[k] for r in rows) for k in range(3)))
assert list(got) == [r[3] for r in rows] and len(rows) > 1000
assert B.host_fallback_rounds() == 0
print("ok")
"""


@pytest.mark.skipif(not os.path.exists(B.LIB_PATH), reason="librbc_amd.so is not built")
def test_product_library_verifies_taproot_without_a_device():
    """librbc_amd.so with the threshold above every batch and every GPU hidden from the child:
    bcc_taproot_verify_batch over all golden checks, bcc_verify_input on a key-path and a
    script-path spend, and mi_schnorr_verify_tuples: golden answers, no device opened."""
    env = dict(os.environ, BCC_HOST_SMALL_ROUND=str(H.HOST_ALL), HIP_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", _PRODUCT_CHILD, PKG, HERE], capture_output=True,
                       text=True, timeout=300, env=env)
    assert p.returncode == 0 and "ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-2000:])
