"""GPU: the block entries through librbc_amd.so with every round a device round
(bcc_set_host_small_round(0), the suite's setting): tx_hash_kernel and merkle_level_kernel on every
case of tests/block_model.py, each result compared with the model and with the engine's host
route.  The injected faults fail a round before it is launched, so nothing here makes the GPU
fail; they run in a child process, as the other failure tests do, because a host fallback is what
they are about."""
import os
import subprocess
import sys

import pytest

import bitcoinconsensus_amd as B
import block_commit_checks as K
import block_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(HERE, "..", "rust-bitcoinconsensus_amd")


def test_tx_hashes():
    """Full and stripped lengths with len mod 64 in {0, 1, 55, 56, 63}, 64 consecutive lengths with
    and without witness data, no outputs, 253 inputs, items that do not parse between good ones."""
    K.check_tx_hashes(None)


def test_long_transaction_and_the_long_chain_threshold():
    K.check_long_tx(None)


def test_round_cuts_inside_a_batch():
    K.check_round_cuts(None)


def test_merkle_roots():
    K.check_merkle(None)


def test_blocks():
    K.check_blocks(None)


def test_two_entries_of_one_device_equal_the_single_device():
    B.set_devices([0, 0])
    try:
        K.check_blocks(None, devices=[0, 0])
        raws = [raw for _, raw, _ in K.tx_batch()] * 3
        with K.settings(None):
            one = B.tx_hashes(raws, device=0)
            assert B.tx_hashes(raws, device=-1) == one
            assert B.last_block_stats()["device_rounds"] == 2
    finally:
        B.set_devices([0])


def test_thread_state_is_released_and_rebuilt():
    blocks = [(raw, sw) for _, raw, sw in M.block_cases()[:8]]
    with K.settings(None):
        want = B.block_commitments(blocks)
        B.release_thread_state()
        assert B.block_commitments(blocks) == want


_FAULTS_CHILD = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import bitcoinconsensus_amd as B
import block_commit_checks as K
assert K.has_kernels(None)
assert K.fault_sequence(None)
print("ok")
"""


def test_injected_faults_retry_fall_back_and_report():
    p = subprocess.run([sys.executable, "-c", _FAULTS_CHILD, PKG, HERE], capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, BCC_HOST_SMALL_ROUND="0"))
    assert p.returncode == 0 and "ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-3000:])
