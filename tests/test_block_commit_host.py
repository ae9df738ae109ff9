"""CPU: the block entries (bcc_tx_hashes_batch, bcc_merkle_root, bcc_block_commitments_batch) in the
device-less engine build (tests/engine_stub.py), where a device round is the host evaluation behind
the device seam: the parser, the job records, the round cuts, the comparisons, the failure rules
and the statistics, every case of tests/block_model.py against the model.  The merkle lane code
and level tables of the kernels, and the rebase rule of TxHashJob, run on the CPU through
tests/native/block_host.cpp (test-only).  The -m gpu twin is test_block_commit_gpu.py."""
import ctypes
import os
import random
import subprocess

import pytest

import bitcoinconsensus_amd as B
import block_commit_checks as K
import block_model as M
import engine_stub
import sighash_model as SM
from oracle_ctypes import Oracle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-bitcoinconsensus_amd", "csrc")
SO = os.path.join(HERE, "native", "_build", "block_host.so")
REF_BLOCK = "/root/reference/depend/bitcoin/src/bench/data/block413567.raw"


@pytest.fixture(scope="module")
def L():
    return K.bind(engine_stub.load())


@pytest.fixture(scope="module")
def host():
    engine_stub.load()  # builds engine_host.so: the engine's host code this library links
    src = os.path.join(HERE, "native", "block_host.cpp")
    deps = [src, engine_stub.SO] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        tmp = SO + f".{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread",
                               "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", tmp, src,
                               engine_stub.SO, "-Wl,-rpath," + os.path.dirname(SO)])
        os.replace(tmp, SO)
    H = ctypes.CDLL(SO)
    H.block_host_merkle_lanes.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint), ctypes.c_uint,
                                          ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
    H.block_host_rebase.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint),
                                    ctypes.c_uint, ctypes.POINTER(ctypes.c_uint), ctypes.c_uint] + \
                                   [ctypes.c_char_p] * 4
    H.block_host_chain_blocks.argtypes = [ctypes.c_uint] * 3
    H.block_host_chain_blocks.restype = ctypes.c_uint
    return H


def test_model_digests_agree_with_the_oracle():
    """hashlib against the oracle's SHA-256d on the messages the model hashes: the stripped and the
    full serializations, a 64-byte node, the commitment message."""
    O = Oracle()
    rng = random.Random(M.SEED)
    msgs = [b"", rng.randbytes(64), rng.randbytes(55), rng.randbytes(56), rng.randbytes(119)]
    for _, raw in M.tx_cases()[::7]:
        t = M.Tx(raw)
        msgs += [t.stripped(), t.raw]
    msgs.append(M.long_tx())
    for m in msgs:
        assert O.sha256d(m) == M.sha256d(m), len(m)


def test_model_strips_marker_flag_and_witnesses():
    rng = random.Random(M.SEED + 6)
    for nin, outs in ((1, (25,)), (3, (25, 23)), (2, ()), (253, (22,))):
        plain = SM.rand_tx(rng, nin, outs)
        t = SM.parse_tx(plain)
        wit = SM.ser_tx(t["version"], t["vin"], t["vout"], t["locktime"],
                        [[rng.randbytes(1 + k)] for k in range(nin)])
        assert M.Tx(wit).stripped() == plain and M.Tx(plain).stripped() == plain
        assert M.tx_hashes(wit)[0] == M.tx_hashes(plain)[0] == M.sha256d(plain)
        assert M.tx_hashes(wit)[1] == M.sha256d(wit) != M.tx_hashes(wit)[0]


def test_fixture_leaves_give_the_header_root():
    header, n, txids = M.load_fixture()
    assert len(header) == 80 and n == len(txids) == 1557 and len(set(txids)) == n
    assert M.merkle_root(txids) == (header[36:68], False)


def test_tx_hashes(L):
    K.check_tx_hashes(L)


def test_long_transaction_and_the_long_chain_threshold(L):
    K.check_long_tx(L)


def test_round_cuts_inside_a_batch(L):
    K.check_round_cuts(L)


def test_merkle_roots(L):
    K.check_merkle(L)


def test_blocks(L):
    K.check_blocks(L)


def test_blocks_over_a_device_list(L):
    engine_stub.set_devices(L, [0, 0])
    try:
        K.check_blocks(L, devices=[0, 0])
        raws = [raw for _, raw, _ in K.tx_batch()] * 3
        with K.settings(L):
            one = B.tx_hashes(raws, device=0, library=L)
            assert B.tx_hashes(raws, device=-1, library=L) == one
            assert B.last_block_stats(library=L)["device_rounds"] == 2
    finally:
        engine_stub.set_devices(L, [0])


def test_injected_faults_retry_fall_back_and_report(L):
    assert K.fault_sequence(L)


def test_thread_state_is_released_and_rebuilt(L):
    blocks = [(raw, sw) for _, raw, sw in M.block_cases()[:8]]
    with K.settings(L):
        want = B.block_commitments(blocks, library=L)
        L.bcc_release_thread_state()
        assert B.block_commitments(blocks, library=L) == want


@pytest.mark.skipif(not os.path.exists(REF_BLOCK), reason="the reference tree is not on this machine")
def test_reference_block_through_block_commitments(L):
    raw = open(REF_BLOCK, "rb").read()
    header, n, txids = M.load_fixture()
    assert raw[:80] == header
    for route, kw in K.routes(L):
        with K.settings(L, **kw):
            got = B.block_commitments([(raw, 0)], library=L)[0]
            st = B.last_block_stats(library=L)
        assert got["status"] == B.BLOCK_OK and got["n_tx"] == n and got["commit_pos"] == -1
        assert got["merkle_root"] == header[36:68] and got["txids"] == txids
        assert st["txs"] == n and st["blocks"] == 1
        K.expect_route(st, route, rounds=1)
    # ... and its transactions through tx_hashes (none carries witness data: wtxid == txid)
    with K.settings(L):
        pos, items = 83, []
        for _ in range(n):
            t = M.Tx(raw, pos)
            items.append(t.raw)
            pos = t.end
        assert pos == len(raw)
        tx, wtx, err = B.tx_hashes(items, library=L)
        assert tx == txids and wtx == txids and not any(err)


def test_merkle_lane_code_and_level_tables(host):
    """The kernels' lane code, launched level by level as block_hash.hip does, one tree at a time
    and many trees in one launch sequence."""
    cases = [(label, lv) for label, lv in M.merkle_cases() if lv]

    def run(trees):
        n = (ctypes.c_uint * len(trees))(*[len(t) for t in trees])
        roots = ctypes.create_string_buffer(32 * len(trees))
        mut = (ctypes.c_int * len(trees))()
        launches = host.block_host_merkle_lanes(b"".join(b"".join(t) for t in trees), n, len(trees),
                                                roots, mut)
        return launches, [(roots.raw[32 * k: 32 * k + 32], bool(mut[k])) for k in range(len(trees))]

    for label, lv in cases:
        launches, got = run([lv])
        assert got == [M.merkle_root(lv)], label
        assert launches == max(1, (len(lv) - 1).bit_length()), label
    launches, got = run([lv for _, lv in cases])
    assert got == [M.merkle_root(lv) for _, lv in cases]
    assert launches == 10  # the 1000-leaf tree's
    header, n, txids = M.load_fixture()
    assert run([txids])[1] == [(header[36:68], False)]


def test_rebase_of_tx_hash_jobs_under_concatenation(host):
    """Three parts (the middle one empty, witness and plain transactions in both others): every
    part alone and the rebased merge give the model's digests."""
    raws = [raw for _, raw in M.tx_cases()[::5]] + [M.long_tx()]
    random.Random(M.SEED + 7).shuffle(raws)
    n = len(raws)
    cut = [0, n // 3, n // 3, n]
    arr = (ctypes.c_char_p * n)(*raws)
    lens = (ctypes.c_uint * n)(*[len(r) for r in raws])
    part = (ctypes.c_uint * len(cut))(*cut)
    bufs = [ctypes.create_string_buffer(32 * n) for _ in range(4)]
    assert host.block_host_rebase(arr, lens, n, part, len(cut) - 1, *bufs) == 0
    want_t = b"".join(M.tx_hashes(r)[0] for r in raws)
    want_w = b"".join(M.tx_hashes(r)[1] for r in raws)
    assert {M.Tx(r).extended for r in raws[:cut[1]]} == {M.Tx(r).extended for r in raws[cut[2]:]} == \
        {False, True}
    assert bufs[0].raw == bufs[2].raw == want_t and bufs[1].raw == bufs[3].raw == want_w


def test_chain_length_of_a_record(host):
    """What bcc_set_host_txhash_blocks is compared with: the blocks of the job's longest lane."""
    f = host.block_host_chain_blocks
    TXH_W, TXH_WZERO = 2, 4
    assert f(55, 0, 0) == 1 and f(56, 0, 0) == 2 and f(119, 0, TXH_W) == 2 and f(120, 0, TXH_W) == 3
    # a witness transaction: the stripped bytes (wit + 2) without a wtxid lane, else every byte
    assert f(1000, 100, 0) == f(102, 0, 0) == 2
    assert f(1000, 100, TXH_W) == f(1000, 0, 0) == 16
    assert f(1000, 100, TXH_W | TXH_WZERO) == 2


def test_python_structs_match_c_layout(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bcc_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(bcc_tx_ref),'
                   ' sizeof(bcc_block_ref), offsetof(bcc_block_ref, txid_cap), sizeof(bcc_block_result),'
                   ' offsetof(bcc_block_result, witness_root), sizeof(bcc_block_stats),'
                   ' offsetof(bcc_block_stats, device_retries)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(B.TxRef), ctypes.sizeof(B.BlockRef), B.BlockRef.txid_cap.offset,
                   ctypes.sizeof(B.BlockResult), B.BlockResult.witness_root.offset,
                   ctypes.sizeof(B.BlockStats), B.BlockStats.device_retries.offset]
