"""CPU: bcc_verify_inputs_batch / bcc_verify_input (csrc/host/inputs.cpp: the flag rule, the
transaction and spent-output rules, locating spent[n_in], the stable partition onto the two engines
and the scatter of their answers) in the device-less engine build (tests/engine_stub.py), against
the cases of tests/mixed_input_cases.py: the 4,207 lifted script cases, the Taproot goldens under
both flag sets, the mixed transactions of tests/golden/mixed_inputs.json.gz and the contract cases.
The -m gpu twin (test_inputs_gpu.py) runs the same cases through librbc_amd.so."""
import ctypes
import random

import pytest

import bitcoinconsensus_amd as B
import engine_stub
import mixed_input_cases as M


@pytest.fixture(scope="module")
def L():
    lib = engine_stub.load()
    ip = ctypes.POINTER(ctypes.c_int)
    lib.bcc_verify_inputs_batch.argtypes = [ctypes.POINTER(B.InputItem), ctypes.c_size_t,
                                            ctypes.c_uint, ip, ip]
    lib.bcc_verify_inputs_batch.restype = ctypes.c_long
    lib.bcc_verify_input.argtypes = [ctypes.c_char_p, ctypes.c_uint, ctypes.c_char_p, ctypes.c_uint,
                                     ctypes.c_uint, ctypes.c_uint, ip]
    lib.bcc_last_inputs_stats.argtypes = [ctypes.POINTER(B.InputsStats)]
    return lib


CLASSES = {"lifted": M.lifted_cases, "taproot": M.taproot_cases, "mixed": M.mixed_cases,
           "contract": M.all_contract_cases}


def by_flags(cases):
    """{flags: [index]} in case order."""
    out = {}
    for i, c in enumerate(cases):
        out.setdefault(c["flags"], []).append(i)
    return out


def run_batches(cases, library=None, stats=False):
    """Every case through one batch per flag set; returns the answers in case order (and, with
    stats, checks the routing counts of every batch)."""
    got = [None] * len(cases)
    for flags, idx in by_flags(cases).items():
        sub = [cases[i] for i in idx]
        rc, res = B.verify_inputs_batch_raw(M.items_of(sub), flags, library=library)
        assert rc == sum(r == 1 for r, _ in res), (flags, rc)
        for i, r in zip(idx, res):
            got[i] = r
        if stats:
            st = B.last_inputs_stats(library=library)
            assert st["items"] == len(sub)
            assert st["ecdsa_side_items"] + st["taproot_side_items"] + st["host_decided_items"] == len(sub)
            # a silent mis-route would show here even where both engines answer alike
            assert st["taproot_side_items"] == sum(c["v1"] for c in sub), (flags, st)
            decided = sum(c["expected"][1] != 0 for c in sub)
            assert st["host_decided_items"] == decided, (flags, st)
    return got


def check(got, cases):
    bad = [(i, c["cls"], hex(c["flags"]), tuple(g), c["expected"])
           for i, (g, c) in enumerate(zip(got, cases)) if tuple(g) != tuple(c["expected"])]
    assert len(got) == len(cases) and not bad, bad[:10]


def test_case_classes_cover_what_the_issue_lists():
    lifted = M.lifted_cases()
    assert sum(not c["cls"].startswith("lifted_tr:") for c in lifted) == 4207
    assert sum(c["cls"].startswith("lifted_tr:") for c in lifted) == 1491
    tap = M.taproot_cases()
    assert len(tap) == 2 * 216 and sum(c["expected"] == (1, 0) and c["v1"] for c in tap) == 90
    txs = M.mixed_txs()
    assert len(txs) >= 40 and all(2 <= len(t["inputs"]) <= 4 for t in txs)
    both = sum(len({i["kind"] in M.V1_KINDS for i in t["inputs"]}) == 2 for t in txs)
    assert 4 * both >= 3 * len(txs)
    ins = [i for t in txs for i in t["inputs"]]
    assert 0.3 * len(ins) <= sum(i["ret"] for i in ins) <= 0.7 * len(ins)
    for kind in M.KINDS:
        assert {i["ret"] for i in ins if i["kind"] == kind} == {0, 1}, kind
    # the cross-kind effect: another input's scriptPubKey changed after signing
    assert any(any((x or "").startswith("other_spk") for x in t["tamper"]) and
               0 in [i["ret"] for i in t["inputs"] if i["kind"] in M.V1_KINDS] and
               1 in [i["ret"] for i in t["inputs"] if i["kind"] not in M.V1_KINDS] for t in txs)
    errs = {c["expected"] for c in M.all_contract_cases()}
    assert {(0, 1), (0, 2), (0, 3), (0, 5), (0, 7), (0, 0), (1, 0)} <= errs


@pytest.mark.parametrize("name", list(CLASSES))
def test_class_as_batches(L, name):
    cases = CLASSES[name]()
    check(run_batches(cases, library=L, stats=True), cases)


@pytest.mark.parametrize("name", list(CLASSES))
def test_class_one_item_per_call(L, name):
    cases = CLASSES[name]()
    if name == "lifted":
        cases = cases[::5]  # ~1,100 single calls: every fifth of the rows and their TAPROOT twins
    got = [B.verify_input(c["tx"], c["spent"], c["nin"], c["flags"], library=L) for c in cases]
    check(got, cases)


def test_single_call_stats_and_null_buffers(L):
    c = next(c for c in M.mixed_cases() if c["v1"])
    assert B.verify_input(c["tx"], c["spent"], c["nin"], c["flags"], library=L) == c["expected"]
    st = B.last_inputs_stats(library=L)
    assert (st["items"], st["taproot_side_items"], st["ecdsa_side_items"]) == (1, 1, 0)
    e = ctypes.c_int(-1)
    f = M.ALL | M.TAPROOT
    assert L.bcc_verify_input(None, 0, c["spent"], len(c["spent"]), 0, f, ctypes.byref(e)) == 0
    assert e.value == M.ERR_TX_DESERIALIZE
    assert L.bcc_verify_input(c["tx"], len(c["tx"]), None, 0, c["nin"], f, ctypes.byref(e)) == 0
    assert e.value == M.ERR_SPENT_OUTPUTS_MISMATCH
    assert L.bcc_verify_input(c["tx"], len(c["tx"]), c["spent"], len(c["spent"]), c["nin"], f,
                              None) == c["expected"][0]


def test_empty_null_and_return_count(L):
    fn = L.bcc_verify_inputs_batch
    f = M.ALL | M.TAPROOT
    ret, err = (ctypes.c_int * 2)(7, 7), (ctypes.c_int * 2)(7, 7)
    assert fn(None, 0, f, None, None) == 0
    assert fn(None, 1, f, ret, err) == -1
    one = (B.InputItem * 2)()
    assert fn(one, 1, f, None, err) == -1
    assert fn(one, 1, f, ret, err) == -1  # null tx and spent_outputs
    cs = [c for c in M.mixed_cases() if c["expected"] == (1, 0)][:2]
    one[0] = B.InputItem(cs[0]["tx"], len(cs[0]["tx"]), cs[0]["spent"], len(cs[0]["spent"]), cs[0]["nin"])
    one[1] = B.InputItem(cs[1]["tx"], len(cs[1]["tx"]), None, 0, cs[1]["nin"])
    assert fn(one, 2, f, ret, err) == -1
    assert list(ret) == [7, 7] and list(err) == [7, 7]  # nothing was verified
    one[1] = B.InputItem(cs[1]["tx"], len(cs[1]["tx"]), cs[1]["spent"], len(cs[1]["spent"]), cs[1]["nin"])
    assert fn(one, 2, f, ret, None) == 2 and list(ret) == [1, 1]  # err_out may be NULL
    mixed = M.mixed_cases()
    rc, res = B.verify_inputs_batch_raw(M.items_of(mixed), f, library=L)
    assert rc == sum(c["expected"][0] for c in mixed) and 0 < rc < len(mixed)
    # invalid flags: every item, nothing routed
    rc, res = B.verify_inputs_batch_raw(M.items_of(mixed), M.TAPROOT, library=L)
    assert rc == 0 and res == [(0, M.ERR_INVALID_FLAGS)] * len(mixed)
    st = B.last_inputs_stats(library=L)
    assert (st["host_decided_items"], st["ecdsa_side_items"], st["taproot_side_items"]) == (len(mixed), 0, 0)


def pool_cases():
    """Mixed, Taproot and contract cases under the full flag set, and a slice of the lifted ones."""
    f = M.ALL | M.TAPROOT
    out = [c for c in M.mixed_cases() + M.taproot_cases() + M.all_contract_cases() if c["flags"] == f]
    return out + [c for c in M.lifted_cases() if c["flags"] == f][::9]


def test_order_independence(L):
    """The same items shuffled give the same per-item answers: nothing depends on an item's
    neighbours, on which slice of the routing pass it falls in or on where its side's batch is cut."""
    cases = pool_cases()
    f = M.ALL | M.TAPROOT
    base = B.verify_inputs_batch(M.items_of(cases), f, library=L)
    check(base, cases)
    for seed in (1, 2):
        order = list(range(len(cases)))
        random.Random(seed).shuffle(order)
        got = B.verify_inputs_batch(M.items_of([cases[i] for i in order]), f, library=L)
        assert got == [base[i] for i in order]


def test_parts_round_cuts_pipeline_chunks_and_devices(L):
    """More routing slices than one (> 2 x 1024 items), the spend round and the pipeline chunk cut
    small with another thread count, one transaction's four inputs (two of each kind) across both
    cuts, and three devices with more than 4,096 items on either side: all equal to the plain
    answer."""
    cases = pool_cases()
    rng = random.Random(11)
    small = [c for c in cases if len(c["tx"]) < 1500]
    pick = [rng.choice(small) for _ in range(2100)]
    four = next(t for t in M.mixed_txs() if sorted(i["kind"] in M.V1_KINDS for i in t["inputs"]) ==
                [False, False, True, True])
    pick[1500:1500] = M.cases_of_tx(four)
    f = M.ALL | M.TAPROOT
    items = M.items_of(pick)
    base = B.verify_inputs_batch(items, f, library=L)
    check(base, pick)
    st = B.last_inputs_stats(library=L)
    assert st["taproot_side_items"] == sum(c["v1"] for c in pick) and st["ecdsa_side_items"] > 800
    L.bcc_set_pipeline_chunk.argtypes = [ctypes.c_size_t]
    L.bcc_set_host_threads.argtypes = [ctypes.c_uint]
    try:
        B.set_spend_round(300, library=L)
        L.bcc_set_pipeline_chunk(200)
        L.bcc_set_host_threads(3)
        assert B.verify_inputs_batch(items, f, library=L) == base
        L.bcc_set_host_threads(0)
        engine_stub.set_devices(L, [0, 1, 2])
        assert B.verify_inputs_batch(items * 5, f, library=L) == base * 5
        assert B.last_inputs_stats(library=L)["taproot_side_items"] > 4096
    finally:
        engine_stub.set_devices(L, [])
        L.bcc_set_host_threads(0)
        L.bcc_set_pipeline_chunk(500_000)
        B.set_spend_round(0, library=L)


def test_many_inputs_of_one_transaction_share_one_walk(L):
    """300 inputs of one transaction, every input an item: the answers of the first and the last
    input equal their single calls (the spent outputs are walked per run, not per item)."""
    import taproot_spend_cases as S
    rng = random.Random(5)
    t = S.G.make_tx(rng, nin=300, nout=2, long_ok=False)
    t["vin"] = [(p, b"\x51", s) for p, _, s in t["vin"]]  # scriptSig OP_1 under an empty script
    t["wit"] = None
    t["spent"] = [(k, b"") for k in range(300)]
    tx, spent = S.G.tx_bytes(t), S.G.ser_outs(t["spent"])
    items = [dict(tx=tx, spent=spent, nin=k) for k in range(300)]
    got = B.verify_inputs_batch(items, M.ALL | M.TAPROOT, library=L)
    assert got == [(1, 0)] * 300
    assert B.verify_input(tx, spent, 299, library=L) == (1, 0)
    assert B.verify_input(tx, spent, 300, library=L) == (0, M.ERR_TX_INDEX)


def test_release_thread_state_and_concurrent_callers(L):
    """A mixed call keeps a second caller thread for the v1 side; bcc_release_thread_state releases
    and joins it and the next call starts a fresh one.  Two threads calling at once share nothing."""
    import threading
    cases = pool_cases()
    f = M.ALL | M.TAPROOT
    items = M.items_of(cases)
    base = B.verify_inputs_batch(items, f, library=L)
    check(base, cases)
    L.bcc_release_thread_state()
    L.bcc_release_thread_state()
    assert B.verify_inputs_batch(items, f, library=L) == base
    out = [None, None]

    def work(k):
        for _ in range(2):
            out[k] = B.verify_inputs_batch(items, f, library=L)
        L.bcc_release_thread_state()

    ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert out == [base, base]
