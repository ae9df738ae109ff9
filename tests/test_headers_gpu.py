"""GPU: bcc_headers_batch and mi_pow_check_tuples through librbc_amd.so with every round a device
round (bcc_set_host_small_round(0), the suite's setting): header_hash_kernel,
header_context_kernel and pow_check_kernel on every case of tests/header_cases.py, each result
compared with tests/header_model.py and with the engine's host route.  The injected faults fail a
round before it is launched, so nothing here makes the GPU fail; they run in a child process, as
the other failure tests do, because a host fallback is what they are about."""
import gzip
import json
import os
import subprocess
import sys

import pytest

import bitcoinconsensus_amd as B
import header_cases as K
import header_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(HERE, "..", "rust-bitcoinconsensus_amd")


def test_mainnet_genesis_header():
    with gzip.open(os.path.join(HERE, "golden", "header_cases.json.gz")) as f:
        g = json.load(f)["genesis"]
    h = M.header(g["version"], bytes(32), bytes.fromhex(g["merkle_root"])[::-1], g["time"], g["bits"], g["nonce"])
    with K.settings(None):
        got = B.check_headers([h])
        assert B.last_header_stats() == dict(headers=1, device_rounds=1, host_rounds=0, device_retries=0)
    assert got["status"] == [B.HEADER_OK] and got["first_invalid"] == 1
    assert got["hashes"][0][::-1].hex() == g["hash"] and got["chain_work"] == g["block_proof"]


def test_lane_geometry():
    """n = 1, 63, 64, 65, 257; 40 headers in rounds of 7 and 16; the chain continued from anchors."""
    K.check_lane_geometry(None)


def test_two_entries_of_one_device_equal_the_single_device():
    K.check_device_list(None, B.set_devices)


def test_compact_targets():
    K.check_compact_targets(None)


def test_retargets():
    K.check_retargets(None)


def test_times():
    K.check_times(None)


def test_versions():
    K.check_versions(None)


def test_linkage():
    K.check_linkage(None)


def test_order_and_work():
    K.check_order_and_work(None)


def test_thread_state_is_released_and_rebuilt():
    base = list(K.base_chain())
    with K.settings(None):
        want = K.run(None, base, K.PARAMS)
        B.release_thread_state()
        assert K.run(None, base, K.PARAMS) == want == M.check(base, K.PARAMS)


_FAULTS_CHILD = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import bitcoinconsensus_amd as B
import header_cases as K
assert not hasattr(K.bind(None), "stub_early_checked")
assert K.fault_sequence(None)
print("ok")
"""


def test_injected_faults_retry_fall_back_and_report():
    p = subprocess.run([sys.executable, "-c", _FAULTS_CHILD, PKG, HERE], capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, BCC_HOST_SMALL_ROUND="0"))
    assert p.returncode == 0 and "ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-3000:])
