"""What the block-entry tests share (test_block_commit_host.py on the device-less engine, where a
device round is the host evaluation behind the device seam; test_block_commit_gpu.py on
librbc_amd.so): every case of block_model.py through one build of the C ABI, compared with the
model, with the small-round threshold at 0 (every round a device round) or above every batch (every
round on the host)."""
import contextlib
import ctypes
import random

import bitcoinconsensus_amd as B
import block_model as M
import sighash_model as SM

HOST_ALL = 1 << 30          # a small-round threshold no test batch reaches
LAUNCH_FAILURE = 719        # hipErrorLaunchFailure: never retried
DEFAULT_TXHASH_BLOCKS = B.HOST_TXHASH_BLOCKS_DEFAULT


def bind(L):
    L = B.lib() if L is None else L
    B._bind_consensus(L)
    B._bind_block(L)
    return L


@contextlib.contextmanager
def settings(L, small_round=0, block_round=0, txhash_blocks=DEFAULT_TXHASH_BLOCKS):
    """The thresholds for one block of code; the suite's settings (threshold 0, default rounds and
    long-chain threshold, no injection, the default policy, one device) are restored afterwards."""
    L = bind(L)
    try:
        L.bcc_set_host_small_round(small_round)
        L.bcc_set_block_round(block_round)
        L.bcc_set_host_txhash_blocks(txhash_blocks)
        yield L
    finally:
        L.bcc_debug_fail_device_rounds(0)
        L.bcc_set_device_failure_policy(B.DEVICE_FAILURE_HOST)
        L.bcc_set_block_round(0)
        L.bcc_set_host_txhash_blocks(DEFAULT_TXHASH_BLOCKS)
        L.bcc_set_host_small_round(0)


def routes(L):
    """(name, settings) of the two routes: the device round and the host evaluation."""
    return (("device", dict(small_round=0)), ("host", dict(small_round=HOST_ALL)))


def has_kernels(L):
    """Whether L's device rounds run kernels (librbc_amd.so) or the device-less engine's stand-in,
    which launches nothing and sends no long transaction anywhere."""
    return not hasattr(bind(L), "stub_early_checked")


def expect_route(st, route, rounds=None):
    if route == "device":
        assert st["host_rounds"] == 0 and st["device_rounds"] >= 1, st
    else:
        assert st["device_rounds"] == 0 and st["host_rounds"] >= 1, st
        assert st["host_long_txs"] == 0 and st["merkle_launches"] == 0, st
    if rounds is not None:
        assert st["device_rounds"] + st["host_rounds"] == rounds, st
    assert st["device_retries"] == 0, st


# ------------------------------------------------------------------------------------------------


def tx_batch():
    """The transaction cases with the items that do not parse spread among them."""
    good = M.tx_cases()
    bad = M.bad_tx_cases()
    items = [(label, raw, 0) for label, raw in good]
    step = len(items) // (len(bad) + 1)
    for k, (label, raw, err) in enumerate(bad):
        items.insert((k + 1) * step + k, (label, raw, err))
    return items


def compare_tx(got, items):
    txid, wtxid, err = got
    bad = []
    for i, (label, raw, want_err) in enumerate(items):
        mt, mw, me = M.tx_hashes(raw)
        assert me == want_err, (label, me, want_err)
        if (txid[i], err[i]) != (mt, me) or (wtxid is not None and wtxid[i] != mw):
            bad.append((i, label, err[i], me))
    assert not bad, bad[:10]


def check_tx_hashes(L):
    L = bind(L)
    items = tx_batch()
    raws = [raw for _, raw, _ in items]
    assert len(items) > 170
    for route, kw in routes(L):
        with settings(L, **kw):
            got = B.tx_hashes(raws, library=L)
            st = B.last_block_stats(library=L)
            compare_tx(got, items)
            expect_route(st, route, rounds=1)
            assert st["txs"] == sum(e == 0 for _, _, e in items) and st["blocks"] == 0
            assert st["bytes_hashed"] == sum(len(M.Tx(r).stripped()) + (len(r) if M.Tx(r).extended else 0)
                                             for _, r, e in items if e == 0)
            # txids alone; a lone item; nothing
            only = B.tx_hashes(raws, wtxid=False, library=L)
            assert only[0] == got[0] and only[1] is None and only[2] == got[2]
            for i in (0, len(items) // 2, len(items) - 1):
                one = B.tx_hashes([raws[i]], library=L)
                assert (one[0][0], one[1][0], one[2][0]) == (got[0][i], got[1][i], got[2][i])
            assert B.tx_hashes([], library=L) == ([], [], [])
    f = L.bcc_tx_hashes_batch
    arr = (B.TxRef * 1)(B.TxRef(None, 0))
    assert f(None, 1, None, None, None, 0) == -1 and f(arr, 1, None, None, None, 0) == -1
    assert f(None, 0, None, None, None, 0) == 0


def check_long_tx(L):
    """One transaction of about 40 KB among short ones, with the long-chain threshold above and
    below its chain: the same digests, and on the device route the host-hashed count."""
    L = bind(L)
    long = M.long_tx()
    blocks = (len(long) + 9 + 63) // 64
    raws = [raw for _, raw in M.tx_cases()[:20]] + [long] + [raw for _, raw in M.tx_cases()[20:40]]
    want = [M.tx_hashes(r) for r in raws]
    assert 600 < blocks < 700 and all(e == 0 for _, _, e in want)
    for route, kw in routes(L):
        for th, host_long in ((blocks, 0), (blocks - 1, 1), (0, 0)):
            with settings(L, txhash_blocks=th, **kw):
                got = B.tx_hashes(raws, library=L)
                st = B.last_block_stats(library=L)
            assert list(zip(*got)) == want, (route, th)
            expect_route(st, route, rounds=1)
            on_device = route == "device" and has_kernels(L)
            assert st["host_long_txs"] == (host_long if on_device else 0), (route, th, st)
    # inside a block: the long transaction's txid and wtxid reach the trees on the device
    rng = random.Random(M.SEED + 9)
    nonce = rng.randbytes(32)
    rest = [r for r in raws if M.Tx(r).n_in]
    wroot = M.merkle_root([M.ZERO] + [M.Tx(t).wtxid() for t in rest])[0]
    cb = M.coinbase(rng, [M.commit_out(M.sha256d(wroot + nonce))], [[nonce]])
    blk = M.make_block(rng, [cb] + rest)
    want = M.block_result(blk, 1)
    assert want["status"] == M.OK and want["witness_root"] == wroot
    for route, kw in routes(L):
        with settings(L, txhash_blocks=blocks - 1, **kw):
            got = B.block_commitments([(blk, 1)], library=L)[0]
            st = B.last_block_stats(library=L)
        compare_block(got, want, "long tx in a block")
        assert st["host_long_txs"] == (1 if route == "device" and has_kernels(L) else 0), st


def check_round_cuts(L):
    """300 transactions in rounds of 64: the single-round result, five rounds."""
    L = bind(L)
    rng = random.Random(M.SEED + 5)
    raws = [SM.rand_tx(rng, 1 + k % 3, (25, 23)[:1 + k % 2], witness=bool(k % 2)) for k in range(300)]
    want = [M.tx_hashes(r) for r in raws]
    for route, kw in routes(L):
        with settings(L, **kw):
            whole = B.tx_hashes(raws, library=L)
            expect_route(B.last_block_stats(library=L), route, rounds=1)
        with settings(L, block_round=64, **kw):
            cut = B.tx_hashes(raws, library=L)
            st = B.last_block_stats(library=L)
        assert cut == whole and list(zip(*whole)) == want
        expect_route(st, route, rounds=5)
        assert st["txs"] == 300


def check_merkle(L):
    L = bind(L)
    cases = M.merkle_cases()
    assert {len(lv) for _, lv in cases} >= set(M.MERKLE_SIZES)
    for route, kw in routes(L):
        with settings(L, **kw):
            for label, leaves in cases:
                got = B.merkle_root(leaves, library=L)
                assert got == M.merkle_root(leaves), (route, label)
                st = B.last_block_stats(library=L)
                if leaves:
                    expect_route(st, route, rounds=1)
                    levels = max(1, (len(leaves) - 1).bit_length())
                    on_device = route == "device" and has_kernels(L)
                    assert st["merkle_launches"] == (levels if on_device else 0), (label, st)
                    assert st["txs"] == len(leaves) and st["blocks"] == 1
            by = dict(cases)
            assert (B.merkle_root(by["[a,b,c]"], library=L)[0] ==
                    B.merkle_root(by["[a,b,c,c]"], library=L)[0])
            header, n, txids = M.load_fixture()
            assert len(txids) == n == 1557
            assert B.merkle_root(txids, library=L) == (header[36:68], False)
    f = L.bcc_merkle_root
    root = ctypes.create_string_buffer(b"\xee" * 32, 32)
    assert f(None, 0, root, None, 0) == 0 and root.raw == bytes(32)
    assert f(None, 1, root, None, 0) == -1 and f(b"\0" * 32, 1, None, None, 0) == -1
    assert f(b"\x07" * 64, 2, root, None, 0) == 0  # a null `mutated` is allowed


def compare_block(got, want, label):
    for k in ("status", "n_tx", "commit_pos", "merkle_root", "witness_root", "txids"):
        assert got[k] == want[k], (label, k, got[k] if k in ("status", "n_tx", "commit_pos") else "...",
                                   want[k] if k in ("status", "n_tx", "commit_pos") else "...")


def check_blocks(L, devices=None):
    L = bind(L)
    cases = M.block_cases()
    want = [M.block_result(raw, sw) for _, raw, sw in cases]
    assert {w["status"] for w in want} == set(range(8))
    assert {1, 2, 3, 65, 300} <= {w["n_tx"] for w in want}
    assert any(any(w["witness_root"]) for w in want)
    blocks = [(raw, sw) for _, raw, sw in cases]
    for route, kw in routes(L):
        with settings(L, **kw):
            got = B.block_commitments(blocks, device=0 if devices is None else -1, library=L)
            st = B.last_block_stats(library=L)
            for g, w, (label, _, _) in zip(got, want, cases):
                compare_block(g, w, label)
            if devices is None:
                expect_route(st, route, rounds=1)
            assert st["blocks"] == len(cases) and st["txs"] == sum(w["n_tx"] for w in want)
            # round cuts between blocks, and one block at a time
            L.bcc_set_block_round(64)
            cut = B.block_commitments(blocks, library=L)
            st = B.last_block_stats(library=L)
            L.bcc_set_block_round(0)
            assert cut == got and st["device_rounds"] + st["host_rounds"] >= 6, st
            for i in (0, 4, 7, 9, len(cases) - 1):
                assert B.block_commitments([blocks[i]], library=L) == [got[i]], cases[i][0]
            # a txid buffer that is too small: nothing written, the result unchanged
            i = next(k for k, w in enumerate(want) if w["n_tx"] == 65)
            small = B.block_commitments([blocks[i]], txid_cap=64, library=L)[0]
            assert small["txids"] is None and set(small["txid_buffer"]) == {0xEE}
            assert {k: small[k] for k in got[i] if not k.startswith("txid")} == \
                   {k: got[i][k] for k in got[i] if not k.startswith("txid")}
            exact = B.block_commitments([blocks[i]], txid_cap=65, library=L)[0]
            assert exact["txids"] == want[i]["txids"]
            none = B.block_commitments([blocks[i]], txids=False, library=L)[0]
            assert none["merkle_root"] == want[i]["merkle_root"]
    f = L.bcc_block_commitments_batch
    res = (B.BlockResult * 1)()
    arr = (B.BlockRef * 1)(B.BlockRef(None, 0, 1, None, 0))
    assert f(None, 1, res, 0) == -1 and f(arr, 1, None, 0) == -1 and f(arr, 1, res, 0) == -1
    assert f(None, 0, None, 0) == 0


def fault_sequence(library=None):
    """bcc_debug_fail_device_rounds against the block entries' rounds: one fault is retried, two
    fall back to the host, a sticky code goes straight to the host, and BCC_DEVICE_FAILURE_ERROR
    returns -1; every delivered result is the model's."""
    cases = M.block_cases()
    blocks = [(raw, sw) for _, raw, sw in cases]
    want = [M.block_result(raw, sw) for _, raw, sw in cases]
    raws = [raw for _, raw in M.tx_cases()]
    tx_want = [M.tx_hashes(r) for r in raws]
    leaves = dict(M.merkle_cases())["n=257"]
    with settings(library) as L:
        def run_blocks():
            got = B.block_commitments(blocks, library=L)
            for g, w, (label, _, _) in zip(got, want, cases):
                compare_block(g, w, label)

        def run_txs():
            assert list(zip(*B.tx_hashes(raws, library=L))) == tx_want

        def run_merkle():
            assert B.merkle_root(leaves, library=L) == M.merkle_root(leaves)

        for run in (run_blocks, run_txs, run_merkle):
            for inject, retries, host_rounds in (
                    (lambda: None, 0, 0),
                    (lambda: L.bcc_debug_fail_device_rounds(1), 1, 0),
                    (lambda: L.bcc_debug_fail_device_rounds(2), 1, 1),
                    (lambda: L.bcc_debug_fail_device_rounds_code(1, LAUNCH_FAILURE), 0, 1),
                    (lambda: L.bcc_debug_fail_device_rounds_code(1 << 20, LAUNCH_FAILURE), 0, 1)):
                before = L.bcc_host_fallback_rounds()
                inject()
                try:
                    run()
                finally:
                    L.bcc_debug_fail_device_rounds(0)
                st = B.last_block_stats(library=L)
                assert (st["device_retries"], st["host_rounds"]) == (retries, host_rounds), (run.__name__, st)
                assert st["device_rounds"] == 1 - host_rounds, (run.__name__, st)
                assert L.bcc_host_fallback_rounds() - before == host_rounds
            L.bcc_set_device_failure_policy(B.DEVICE_FAILURE_ERROR)
            before = L.bcc_host_fallback_rounds()
            L.bcc_debug_fail_device_rounds(3)
            try:
                try:
                    run()
                    raise AssertionError("no error under BCC_DEVICE_FAILURE_ERROR")
                except RuntimeError:
                    pass
            finally:
                L.bcc_debug_fail_device_rounds(0)
                L.bcc_set_device_failure_policy(B.DEVICE_FAILURE_HOST)
            assert L.bcc_host_fallback_rounds() == before
            run()  # the next call, with no injection, is whole again
            st = B.last_block_stats(library=L)
            assert (st["device_retries"], st["host_rounds"]) == (0, 0), st
    return True
