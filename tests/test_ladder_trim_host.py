"""CPU: the ladders' trimmed forms (csrc/ecdsa_twist.h: the affine + affine first addition of the Q
ladder and of the comb, the signed Q-table read) against the general forms they replace, by the
stand-alone program tests/native/ladder_trim_host.cpp -- test-only, never part of the product.  The
program compares Jacobian coordinates, infinity flags and verdicts; this file feeds it the
reference fixtures test_lane_host.py uses and builds it a second time under the host sanitizers."""
import os
import subprocess

import pytest

from fixtures import (bip340_vectors, ecdsa_tuples, pub_to_tuple, schnorr_exceptional,
                      schnorr_tuples, structured_scalars)
from oracle_ctypes import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "native", "_build")
SRC = os.path.join(HERE, "native", "ladder_trim_host.cpp")
CSRC = os.path.join(HERE, "..", "rust-bitcoinconsensus_amd", "csrc")
FORMS = {
    "plain": ["-O2"],
    # host sanitizers on the stand-alone program (nothing is loaded into Python)
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


def _build(form):
    exe = os.path.join(BUILD, "ladder_trim_host_" + form)
    deps = [SRC] + [os.path.join(CSRC, f) for f in (
        "ecdsa_lane.h", "ecdsa_twist.h", "secp256k1_device.h", "modinv_host.h", "modinv_device.h",
        "sha256_device.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", *FORMS[form], "-o", exe, SRC, "-lpthread"])
    return exe


@pytest.fixture(scope="module", params=sorted(FORMS))
def prog(request):
    return request.param, _build(request.param)


def _run(exe, *args):
    p = subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    return p.stdout


@pytest.fixture(scope="module")
def ecdsa_rows():
    """Every class of ecdsa_tuples() and every row of the structured-scalar fixture as
    tag | x | y | r | s | m | verdict."""
    O = Oracle()
    rows = []
    ts = ecdsa_tuples()
    for t in ts:
        tag, x, y = pub_to_tuple(t["pub"])
        ok, r, s = O.der_parse_lax(t["sig"])
        if not ok:
            r = s = bytes(32)
        rows.append(bytes([tag]) + x + y + r + s + t["hash"] + bytes([t["verdict"]]))
    assert len({t["cls"] for t in ts}) > 10
    # every third structured row of each class (the host lane tests run them all)
    seen = {}
    for t in structured_scalars()["ecdsa"]:
        k = seen[t["cls"]] = seen.get(t["cls"], -1) + 1
        if k % 3:
            continue
        tag, x, y = pub_to_tuple(t["pub"])
        rows.append(bytes([tag]) + x + y + t["r32"] + t["s32"] + t["hash"] + bytes([t["verdict"]]))
    assert all(len(r) == 162 for r in rows)
    return rows


@pytest.fixture(scope="module")
def schnorr_rows():
    ts = bip340_vectors() + schnorr_tuples() + schnorr_exceptional() + structured_scalars()["schnorr"]
    rows = [t["sig"] + t["msg"] + t["pub"] + bytes([t["verdict"]]) for t in ts]
    assert all(len(r) == 129 for r in rows)
    return rows


def _thin(form, rows):
    # the sanitized build runs several times slower: every eighth row there
    return rows if form == "plain" else rows[::8]


def test_primitive_cases(prog):
    """The first addition with distinct, equal and opposite points, an infinity accumulator, every
    digit sign with every table index, every combination of half signs and corrections, u1 zero /
    even / odd."""
    out = _run(prog[1], "prims")
    assert "prims: 0 failures" in out, out


def test_ecdsa_fixtures_old_against_new(prog, ecdsa_rows, tmp_path):
    form, exe = prog
    rows = _thin(form, ecdsa_rows)
    f = tmp_path / "ecdsa.bin"
    f.write_bytes(b"".join(rows))
    out = _run(exe, "ecdsa", str(f))
    assert f"ecdsa: {len(rows)} rows" in out and " 0 failures" in out, out


def test_schnorr_fixtures_old_against_new(prog, schnorr_rows, tmp_path):
    form, exe = prog
    rows = _thin(form, schnorr_rows)
    f = tmp_path / "schnorr.bin"
    f.write_bytes(b"".join(rows))
    out = _run(exe, "schnorr", str(f))
    assert f"schnorr: {len(rows)} rows" in out and " 0 failures" in out, out
