"""GPU: bcc_tx_check_batch and bcc_block_check_batch through librbc_amd.so with every round a
device round (bcc_set_host_small_round(0), the suite's setting): tx_rules_kernel, dup_input_kernel
and block_rules_kernel on every case of tests/block_rules_cases.py, each result compared with
tests/block_rules_model.py and with the engine's host route.  The injected faults fail a round
before it is launched, so nothing here makes the GPU fail; they run in a child process, as the other
failure tests do, because a host fallback is what they are about."""
import os
import subprocess
import sys

import pytest

import bitcoinconsensus_amd as B
import block_rules_cases as K

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(HERE, "..", "rust-bitcoinconsensus_amd")


def test_transactions():
    """The reference's vectors, the value and sum boundaries, coinbase lengths, null prevouts, every
    edge of the sigop walk in scriptSigs and scriptPubKeys, CompactSize widths, witness data, the
    four alignments; in one round, in rounds of 7, with every and with no transaction on the host."""
    assert K.has_kernels(None)
    K.check_txs(None)


def test_megabyte_transactions():
    K.check_megabyte_txs(None)


def test_duplicate_inputs():
    """2, 3, 64 and 65 inputs with the pair first and last, adjacent and absent; the same outpoint in
    different transactions; chains of colliding slots, one around the table's end; the smallest
    table; a long transaction the host checks during the device round."""
    K.check_duplicates(None)


def test_blocks():
    K.check_blocks(None)


def test_blocks_at_the_size_and_weight_limits():
    K.check_megabyte_blocks(None)


def test_batches_round_cuts_and_a_device_list():
    K.check_batches_and_cuts(None, B.set_devices)


def test_rule_kernel_times_are_reported_or_zero():
    with K.settings(None):
        B.block_check_batch(K.args_of(K.small_blocks()))
        ms = B.block_rules_last_timing_ms()
    assert set(ms) == {"tx_rules_kernel", "dup_input_kernel", "block_rules_kernel", "host_plan", "host_long_txs"}
    assert all(v >= 0 for v in ms.values())


_FAULTS_CHILD = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import bitcoinconsensus_amd as B
import block_rules_cases as K
assert K.has_kernels(None)
assert K.fault_sequence(None)
print("ok")
"""


def test_injected_faults_retry_fall_back_and_report():
    p = subprocess.run([sys.executable, "-c", _FAULTS_CHILD, PKG, HERE], capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, BCC_HOST_SMALL_ROUND="0"))
    assert p.returncode == 0 and "ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-3000:])
