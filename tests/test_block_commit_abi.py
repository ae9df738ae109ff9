"""CPU: the block entries' symbols are declared in include/bcc_amd.h and exported by librbc_amd.so,
the Python wrappers run against the device-less engine build, and the product library answers on
its host route with every GPU hidden."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

import bitcoinconsensus_amd as B
import block_commit_checks as K
import block_model as M
import engine_stub

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "rust-bitcoinconsensus_amd")
SYMBOLS = ("bcc_tx_hashes_batch", "bcc_merkle_root", "bcc_block_commitments_batch",
           "bcc_last_block_stats", "bcc_set_block_round", "bcc_set_host_txhash_blocks",
           "bcc_block_last_timing_ms")


def test_symbols_are_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bcc_amd.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
    for s in ("bcc_tx_ref", "bcc_block_ref", "bcc_block_result", "bcc_block_stats"):
        assert re.search(r"}\s*%s;" % s, header), s
    for k in range(8):
        assert re.search(r"#define BCC_BLOCK_\w+ %d\b" % k, header), k
    if not os.path.exists(B.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", PKG, "-j8"])
    lib = ctypes.CDLL(B.LIB_PATH)
    assert not [s for s in SYMBOLS if not hasattr(lib, s)]
    stub = engine_stub.load()
    assert not [s for s in SYMBOLS if not hasattr(stub, s)]


def test_python_constants_mirror_the_header():
    header = open(os.path.join(ROOT, "include", "bcc_amd.h")).read()
    for name, value in re.findall(r"#define BCC_(BLOCK_\w+) (\d+)", header):
        assert getattr(B, name) == getattr(M, name[6:] if name != "BLOCK_OK" else "OK") == int(value), name


def test_wrappers_against_the_stub_build():
    L = K.bind(engine_stub.load())
    rng_cases = M.tx_cases()[:12]
    raws = [raw for _, raw in rng_cases]
    with K.settings(L, block_round=5, txhash_blocks=3):
        txid, wtxid, err = B.tx_hashes(raws, library=L)
        assert list(zip(txid, wtxid, err)) == [M.tx_hashes(r) for r in raws]
        st = B.last_block_stats(library=L)
        assert set(st) == {"blocks", "txs", "bytes_hashed", "device_rounds", "host_rounds",
                           "host_long_txs", "merkle_launches", "device_retries"}
        assert (st["txs"], st["device_rounds"], st["host_rounds"]) == (12, 3, 0)
        leaves = txid[:7]
        assert B.merkle_root(leaves, library=L) == B.merkle_root(b"".join(leaves), library=L) == \
            M.merkle_root(leaves)
        assert B.merkle_root([], library=L) == (bytes(32), False)
        label, raw, sw = M.block_cases()[7]
        got = B.block_commitments([(raw, sw)], library=L)[0]
        K.compare_block(got, M.block_result(raw, sw), label)
        assert got["status"] == B.BLOCK_OK and got["commit_pos"] >= 0 and any(got["witness_root"])
        ms = B.block_last_timing_ms(library=L)
        assert set(ms) == {"txh_kernel", "merkle_kernels", "upload", "download", "parse", "stage"}
        assert ms["txh_kernel"] == ms["merkle_kernels"] == ms["upload"] == ms["stage"] == 0 < ms["parse"]
    with K.settings(L):
        assert B.last_block_stats(library=L)["txs"] == 7  # the stub's last call: the block's


_PRODUCT_CHILD = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import bitcoinconsensus_amd as B
import block_commit_checks as K
import block_model as M
cases = M.block_cases()
got = B.block_commitments([(raw, sw) for _, raw, sw in cases])
for g, (label, raw, sw) in zip(got, cases):
    K.compare_block(g, M.block_result(raw, sw), label)
st = B.last_block_stats()
assert st["device_rounds"] == 0 and st["host_rounds"] == 1 and st["blocks"] == len(cases), st
raws = [raw for _, raw, _ in K.tx_batch()]
assert list(zip(*B.tx_hashes(raws))) == [M.tx_hashes(r) for r in raws]
for label, leaves in M.merkle_cases():
    assert B.merkle_root(leaves) == M.merkle_root(leaves), label
assert B.last_block_stats()["device_rounds"] == 0
assert B.host_fallback_rounds() == 0
print("ok")
"""


@pytest.mark.skipif(not os.path.exists(B.LIB_PATH), reason="librbc_amd.so is not built")
def test_product_library_on_its_host_route_without_a_device():
    """librbc_amd.so with the small-round threshold on and every GPU hidden from the child: the
    batches below the entries' threshold are evaluated by the host and open no device."""
    env = dict(os.environ, BCC_HOST_SMALL_ROUND="16", HIP_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", _PRODUCT_CHILD, PKG, HERE], capture_output=True,
                       text=True, timeout=300, env=env)
    assert p.returncode == 0 and "ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-2000:])
