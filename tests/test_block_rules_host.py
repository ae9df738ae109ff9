"""CPU: bcc_tx_check_batch and bcc_block_check_batch in the device-less engine build
(tests/engine_stub.py), where a device round is the host evaluation behind the device seam: the
argument rules, the round cuts, the order of the statuses, the failure rules, every case of
tests/block_rules_cases.py against tests/block_rules_model.py; the fixture against the reference's
own data files; and the kernels' lane code as a stand-alone program
(tests/native/block_rules_host.cpp), plainly and under the address and undefined-behaviour
sanitizers.  The -m gpu twin is test_block_rules_gpu.py."""
import ctypes
import os
import random
import re
import subprocess

import pytest

import bitcoinconsensus_amd as B
import block_rules_cases as K
import block_rules_model as M
import engine_stub

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-bitcoinconsensus_amd", "csrc")


@pytest.fixture(scope="module")
def L():
    return K.bind(engine_stub.load())


def test_fixture_pins_the_model():
    K.check_fixture_pins()


def test_model_encodes_heights_as_script_does():
    want = {0: "00", 1: "51", 16: "60", 17: "0111", 127: "017f", 128: "028000", 255: "02ff00", 256: "020001",
            32767: "02ff7f", 32768: "03008000", 8388607: "03ffff7f", 8388608: "0400008000",
            (1 << 31) - 1: "04ffffff7f", -1: "4f", -2: "0182"}
    assert {h: M.push_int(h).hex() for h in want} == want


def test_python_constants_mirror_the_header():
    header = open(os.path.join(ROOT, "include", "bcc_amd.h")).read()
    tx = re.findall(r"#define BCC_(TX_\w+) (\d+)", header)
    blk = re.findall(r"BCC_(BLOCK_\w+) = (\d+)", header)
    assert len(tx) == 10 and len(blk) == 10
    for name, value in tx:
        assert getattr(B, name) == getattr(M, name[7:] if name != "TX_OK" else name) == int(value), name
    for name, value in blk:
        assert getattr(B, name) == getattr(M, name[6:]) == int(value), name


def test_transactions(L):
    K.check_txs(L)


def test_megabyte_transactions(L):
    K.check_megabyte_txs(L)


def test_duplicate_inputs(L):
    K.check_duplicates(L)


def test_blocks(L):
    K.check_blocks(L)


def test_blocks_at_the_size_and_weight_limits(L):
    K.check_megabyte_blocks(L)


def test_batches_round_cuts_and_a_device_list(L):
    K.check_batches_and_cuts(L, lambda devs: engine_stub.set_devices(L, devs))


def test_injected_faults_retry_fall_back_and_report(L):
    assert K.fault_sequence(L)


def test_outpoint_slots_spread_and_depend_on_the_row(L):
    """bcc_debug_outpoint_slot: inside the table, every slot reached, another row another start."""
    for log2 in (1, 2, 3, 8, 31):
        slots = [B.debug_outpoint_slot(5, K.prev(k), log2, library=L) for k in range(4000)]
        assert max(slots) < 1 << log2
        if log2 <= 8:
            assert len(set(slots)) == 1 << log2
    a = [B.debug_outpoint_slot(1, K.prev(k), 16, library=L) for k in range(50)]
    b = [B.debug_outpoint_slot(2, K.prev(k), 16, library=L) for k in range(50)]
    assert a != b and len(set(a)) > 45
    assert [B.debug_dup_table_log2(r, library=L) for r in (0, 1, 2, 3, 4, 5, 64, 65, 1 << 20)] == \
        [1, 1, 2, 3, 3, 4, 7, 8, 21]


def test_python_structs_match_c_layout(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bcc_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(bcc_tx_check_result),'
                   ' offsetof(bcc_tx_check_result, all_final), sizeof(bcc_block_check_ref),'
                   ' offsetof(bcc_block_check_ref, flags), sizeof(bcc_block_check_result),'
                   ' offsetof(bcc_block_check_result, witness_root)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(B.TxCheckResult), B.TxCheckResult.all_final.offset,
                   ctypes.sizeof(B.BlockCheckRef), B.BlockCheckRef.flags.offset,
                   ctypes.sizeof(B.BlockCheckResult), B.BlockCheckResult.witness_root.offset]


def lane_rows():
    """The rows the lane program reads: transactions with the model's record, scripts with their
    count, blocks with the model's sums."""
    rows = []
    for label, script, n in K.script_cases():
        rows.append(f"script {script.hex() or '-'} {n}")
    for label, raw in K.tx_cases():
        r = M.tx_result(raw)
        if r["status"] in (M.ERR_TX_DESERIALIZE, M.ERR_TX_SIZE_MISMATCH):
            continue
        t = M.parse(raw)
        wit = t["stripped_size"] - 2 if t["witness"] is not None else 0
        rows.append(" ".join(str(v) for v in ["tx", raw.hex(), wit, r["status"], r["n_in"], r["n_out"], r["sigops"],
                                                r["lock_time"], r["stripped_size"], r["is_coinbase"], r["all_final"]]))
    for h in (0, 1, 16, 17, 127, 128, 255, 256, 32767, 32768, 65535, 65536, 8388607, 8388608, (1 << 31) - 1):
        rows.append(f"height {h} {M.push_int(h).hex()}")
    rng = random.Random(K.SEED + 3)
    for _ in range(300):  # IsFinalTx around both thresholds
        lock = rng.choice((0, 1, K.HEIGHT - 1, K.HEIGHT, K.HEIGHT + 1, 499999999, 500000000, K.CUTOFF - 1, K.CUTOFF,
                           0xffffffff, rng.randrange(1 << 32)))
        height = rng.choice((0, 1, K.HEIGHT, (1 << 31) - 1))
        cutoff = rng.choice((-1, 0, K.CUTOFF, K.CUTOFF + 1, 1 << 40))
        final = rng.random() < 0.5
        t = dict(lock_time=lock, vin=[(None, None, 0xffffffff if final else 7)])
        rows.append(f"final {lock} {int(final)} {height} {cutoff} {int(M.is_final(t, height, cutoff))}")
    for label, raw, height, cutoff, flags, _ in K.small_blocks():
        r = M.block_result(raw, height, cutoff, flags)
        if r["status"] in (1, 2):
            continue
        n, i = M._compact(raw, 80)
        txs = []
        for _ in range(n):
            t = M.parse(raw, i)
            txs.append(t)
            i = t["end"]
        bad = next((k for k, t in enumerate(txs) if M.check_transaction(t)), -1)
        nonfinal = next((k for k, t in enumerate(txs) if not M.is_final(t, height, cutoff)), -1)
        want = M.push_int(height)
        bip34 = int(bool(txs[0]["vin"]) and txs[0]["vin"][0][1][:len(want)] == want)
        rows.append(" ".join(str(v) for v in [
            "block", raw.hex(), height, cutoff, r["sigops"], sum(t["stripped_size"] for t in txs),
            int(M.is_coinbase(txs[0])), sum(M.is_coinbase(t) for t in txs[1:]), bad,
            M.check_transaction(txs[bad]) if bad >= 0 else 0, nonfinal, bip34, n] +
            [v for t in txs for v in (t["end"] - t["total_size"], t["total_size"],
                                      t["stripped_size"] - 2 if t["witness"] is not None else 0)]))
    return rows


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_lane_program(tmp_path, sanitize):
    """The stand-alone lane program: the lane code through the aligned-dword source the kernels use,
    the plain one and one that asserts every read's bounds, over the fixture and the sweeps; the
    duplicate lane in every arrival order of small tables; 10,000 random byte strings as scripts
    and as transactions.  Nothing is preloaded, the program is its own process."""
    exe = tmp_path / "block_rules_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-O1", "-std=c++17"] + flags +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", str(exe),
                           os.path.join(HERE, "native", "block_rules_host.cpp")])
    rows = lane_rows()
    assert len(rows) > 700
    data = tmp_path / "rows.txt"
    data.write_text("\n".join(rows) + "\n")
    p = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and " 0 mismatches" in p.stdout, (p.returncode, p.stdout, p.stderr[-3000:])
