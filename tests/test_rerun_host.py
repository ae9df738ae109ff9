"""CPU: the engine's second and later device rounds (chunk_stitch, the per-item check
cache, hint_all on re-runs, Round::reset between rounds, the per-transaction state rebuilt when
only some inputs of a transaction re-run) on the verdict-dependent spends of
tests/golden/rerun_cases.json.gz (tests/rerun_cases.py), in the device-less engine build
(tests/engine_stub.py) with every round on the stub device (conftest.py: BCC_HOST_SMALL_ROUND=0).

Expected values are the reference's, recorded in the golden file; rounds_min comes from the
construction.  The -m gpu twin (test_rerun_gpu.py) runs the same cases through librbc_amd.so."""
import ctypes
import os
import random

import pytest

import bitcoinconsensus_amd as B
import engine_stub
import rerun_cases as RC
from oracle_ctypes import reference_available

PIPELINE_CHUNK_DEFAULT = 500_000  # engine.cpp g_pipeline_chunk


@pytest.fixture(scope="module")
def eng():
    L = engine_stub.load()
    L.bitcoinconsensus_verify_batch.argtypes = [ctypes.POINTER(B.BatchItem), ctypes.c_size_t,
                                                ctypes.c_uint, ctypes.POINTER(ctypes.c_int),
                                                ctypes.POINTER(ctypes.c_int)]
    L.bcc_last_batch_stats.argtypes = [ctypes.POINTER(B.BatchStats)]
    L.bcc_set_pipeline_chunk.argtypes = [ctypes.c_size_t]
    L.bcc_set_host_small_round.argtypes = [ctypes.c_size_t]
    for f in ("bcc_set_fused_pass", "bcc_set_early_q", "bcc_set_device_key_hash"):
        getattr(L, f).argtypes = [ctypes.c_int]
    return L


def run(L, cases, flags):
    """One verify_batch call; ([(ret, err)], stats).  Items of one transaction share its buffer."""
    arr, keep = B._batch_items([RC.item(c) for c in cases])
    n = len(cases)
    ret = (ctypes.c_int * n)()
    err = (ctypes.c_int * n)()
    rc = L.bitcoinconsensus_verify_batch(arr, n, flags, ret, err)
    st = B.BatchStats()
    L.bcc_last_batch_stats(ctypes.byref(st))
    got = list(zip(ret, err))
    assert rc == sum(r for r, _ in got)
    del keep
    return got, st


def expected(cases):
    return [(c["ret"], c["err"]) for c in cases]


# ---- the golden file ---------------------------------------------------------------------------
def test_golden_coverage():
    cs = RC.load()
    assert os.path.getsize(RC.GOLDEN) < 535354  # the largest golden file before this one
    for fam in RC.FAMILIES:
        assert {c["ret"] for c in cs if c["family"] == fam} == {0, 1}, fam
    assert {c["family"] for c in cs} == set(RC.FAMILIES)
    assert {c["flags"] for c in cs} == set(RC.FLAG_SETS)
    assert sum(c["rounds_min"] >= 2 for c in cs) >= 200
    assert sum(c["rounds_min"] >= 3 for c in cs) >= 40
    assert sum(c["rounds_min"] == 4 for c in cs) >= 8
    assert max(c["rounds_min"] for c in cs) == 4
    # every (m, n) on its side of the hint bound: a two-round case exists exactly above it
    for m, n in RC.MN:
        ms = [c for c in cs if c["family"] == "multisig" and c["name"].startswith("%dof%d:" % (m, n))]
        assert ms, (m, n)
        assert {c["name"].split(":")[1] for c in ms} == set(RC.signer_sets(m, n)), (m, n)
        assert any(c["rounds_min"] == 2 for c in ms) == RC.above_hint_bound(m, n), (m, n)
        wraps = {c["name"].split(":")[4] for c in ms}
        assert wraps >= set(RC.WRAPPINGS) - ({"p2sh"} if n == 20 else set()), (m, n)
        assert {c["name"].split(":")[3] for c in ms} == set(RC.MS_OPS), (m, n)
        want = set(RC.MS_VARIANTS) - ({"swap", "repeat"} if m < 2 else set())
        assert {c["name"].split(":")[2] for c in ms} == want, (m, n)
    assert all(set(RC.signer_sets(m, n)) == {"first", "last", "alt"} for m, n in RC.MN if 2 <= m <= n // 2)
    assert [RC.above_hint_bound(m, n) for m, n in RC.MN] == [False, False, False, False, True, True,
                                                            False, True, False, False]
    # ladders: every pattern of every depth, bare and P2WSH, and the rounds they were built for
    for d in range(1, 5):
        for w in ("bare", "p2wsh"):
            pats = {c["name"].split(":")[2] for c in cs
                    if c["name"].startswith("ladder:%d:" % d) and c["name"].split(":")[3] == w}
            assert len(pats) == 1 << d, (d, w)
    lad = [c for c in cs if c["name"].startswith("ladder:") and c["flags"] == RC.ALL]
    assert {c["rounds_min"] for c in lad} == {1, 2, 3, 4}
    # all 160 flipped bits, per kind and key form, each a valid signature under the wrong program
    for kind in RC.KH_KINDS:
        for form in RC.KEY_FORMS:
            sweep = [c for c in cs if c["flags"] == RC.ALL and
                     c["name"].startswith("%s:%s:sweep:" % (kind, form))]
            assert sorted(int(c["name"].split(":")[3]) for c in sweep) == list(range(160))
            assert all((c["ret"], c["kh"]) == (0, 1) for c in sweep), (kind, form)
            right = [c for c in cs if c["flags"] == RC.ALL and
                     c["name"] == "%s:%s:right:badsig=0" % (kind, form)]
            assert [c["ret"] for c in right] == [1]
    assert {c["name"].split(":")[2] for c in cs if ":extra" in c["name"]} == {"extra1", "extra98", "extra99"}
    # multi-input: 2-6 inputs, whole transactions and subsets, inputs of unequal round counts
    groups = {}
    for c in cs:
        if c["family"] == "multi_input" and c["flags"] == RC.ALL:
            groups.setdefault(c["group"], []).append(c)
    assert {int(g[0]["name"].split(":")[1]) for g in groups.values()} == {2, 3, 4, 5, 6}
    assert {g[0]["name"].split(":")[3] for g in groups.values()} == {"full", "subset"}
    assert all(len({c["tx"] for c in g}) == 1 for g in groups.values())
    assert sum(len({c["rounds_min"] for c in g}) >= 3 for g in groups.values()) >= 8


@pytest.mark.skipif(not reference_available(), reason="oracle/_ref not built")
def test_golden_equals_a_fresh_reference_run():
    from oracle_ctypes import Reference
    R = Reference()
    for c in RC.load():
        assert R.verify_script_with_amount(*RC.item(c), c["flags"]) == (c["ret"], c["err"]), c["name"]
        ret, _, recs = R.capture_script(*RC.item(c), c["flags"])
        assert ret == c["ret"]
        assert recs == c["checks"], c["name"]


@pytest.mark.skipif(not reference_available(), reason="oracle/_ref not built")
def test_golden_regenerates_byte_for_byte():
    from oracle_ctypes import Oracle, Reference
    with open(RC.GOLDEN, "rb") as f:
        assert RC.dumps(RC.build_all(Reference(), Oracle())) == f.read()


# ---- one-item batches --------------------------------------------------------------------------
@pytest.mark.parametrize("flags", RC.FLAG_SETS)
@pytest.mark.parametrize("family", RC.FAMILIES)
def test_one_item_batches_reach_the_rounds_they_were_built_for(eng, family, flags):
    """Every case alone: the reference's answer, at least rounds_min device rounds (>=, so that a
    future hint that saves a round fails here visibly), and exactly rounds_min for the ladders."""
    bad, hist = [], {}
    cs = [c for c in RC.load() if c["family"] == family and c["flags"] == flags]
    for c in cs:
        got, st = run(eng, [c], flags)
        hist[st.rounds] = hist.get(st.rounds, 0) + 1
        exact = c["name"].startswith("ladder:")
        if (got != [(c["ret"], c["err"])] or st.rounds < c["rounds_min"] or
                (exact and st.rounds != c["rounds_min"])):
            bad.append((c["name"], got, (c["ret"], c["err"]), st.rounds, c["rounds_min"]))
    print("rounds histogram of the one-item batches:", family, hex(flags), sorted(hist.items()))
    assert cs and not bad, (len(bad), bad[:10])
    if family == "ladder":
        assert hist[2] >= 8 and hist[3] >= 4 and hist[4] >= 2  # the rounds they were built for
    if family == "multisig":
        # a re-run is offered every candidate pair (hint_all): never more than one extra round
        assert hist[2] >= 30 and max(hist) == 2


# ---- whole batches -----------------------------------------------------------------------------
def orders(n):
    """File order and two seeded shuffles."""
    out = [list(range(n))]
    for seed in (1, 2):
        o = list(range(n))
        random.Random(seed).shuffle(o)
        out.append(o)
    return out


def check_batches(eng, cases, which, between=None, after=None):
    """The cases of each flag set in one call, in the orders `which` of orders()."""
    for flags, cs in RC.by_flags(cases).items():
        exp = expected(cs)
        for order in [orders(len(cs))[k] for k in which]:
            if between:
                between()
            got, st = run(eng, [cs[i] for i in order], flags)
            bad = [(cs[i]["name"], g, exp[i]) for g, i in zip(got, order) if g != exp[i]]
            assert not bad, (hex(flags), len(bad), bad[:10])
            assert st.rounds >= max(c["rounds_min"] for c in cs) >= 3
            if after:
                after(st)


@pytest.mark.parametrize("flags", RC.FLAG_SETS)
def test_whole_file_in_one_batch(eng, flags):
    """Every case of a flag set in one call, in file order and in two seeded shuffles (on the stub,
    whose device is the plain-C oracle: 9 + 4 + 3 s an order for the three flag sets)."""
    cs = [c for c in RC.load() if c["flags"] == flags]
    assert max(c["rounds_min"] for c in cs) == 4
    check_batches(eng, cs, (0, 1, 2))


def under_setting(eng, between=None, after=None):
    """What runs under every setting: the whole file of each flag set in file order, and
    RC.thin() of it in the two seeded shuffles."""
    check_batches(eng, RC.load(), (0,), between, after)
    check_batches(eng, RC.thin(RC.load()), (1, 2), between, after)


def test_batches_pipelined(eng):
    try:
        eng.bcc_set_pipeline_chunk(61)
        under_setting(eng)
    finally:
        eng.bcc_set_pipeline_chunk(PIPELINE_CHUNK_DEFAULT)


def test_batches_three_devices(eng):
    def after(st):
        assert st.devices == 3
    try:
        engine_stub.set_devices(eng, [0, 1, 2])
        under_setting(eng, after=after)
    finally:
        engine_stub.set_devices(eng, [])


def test_batches_unfused_pass(eng):
    try:
        eng.bcc_set_fused_pass(0)
        under_setting(eng)
    finally:
        eng.bcc_set_fused_pass(1)


@pytest.mark.parametrize("on", [0, 1])
def test_batches_early_q(eng, on):
    try:
        eng.bcc_set_early_q(on)
        under_setting(eng)
    finally:
        eng.bcc_set_early_q(1)


@pytest.mark.parametrize("on", [0, 1])
def test_batches_device_key_hash(eng, on):
    try:
        eng.bcc_set_device_key_hash(on)
        under_setting(eng)
    finally:
        eng.bcc_set_device_key_hash(1)


def test_batches_small_rounds_on_host(eng):
    """Rounds of at most 16 checks in the host lane code: in production usually every round after
    the first."""
    try:
        eng.bcc_set_host_small_round(16)
        under_setting(eng)
    finally:
        eng.bcc_set_host_small_round(int(os.environ.get("BCC_HOST_SMALL_ROUND", "16")))


# device rounds that fail -> (device_retries, host_rounds) of the call: a failed round is retried
# once on a fresh DeviceBatch and verified on the host when the retry fails too
INJECTED = {1: (1, 0),   # round 1 fails, its retry passes
            2: (1, 1),   # round 1 and its retry fail: round 1 on the host
            3: (2, 1),   # ... and round 2, a re-run round, fails once: retried on a fresh batch
            4: (2, 2)}   # ... and its retry fails: a re-run round verified on the host


@pytest.mark.parametrize("fail", list(INJECTED))
def test_batches_with_injected_device_failures(eng, fail):
    """The next `fail` device rounds of a call fail (3 and 4 reach the second round, a re-run round
    stitched through the check cache): the same answers, and the statistics show where the
    failures landed."""
    def inject():
        eng.bcc_debug_fail_device_rounds(fail)

    def after(st):
        assert (st.device_retries, st.host_rounds) == INJECTED[fail]
    try:
        under_setting(eng, inject, after)
    finally:
        eng.bcc_debug_fail_device_rounds(0)


def test_key_hash_near_misses_alone(eng):
    """The key-hash family under 0xE15 in one call with the comparison on the device: the golden
    answers, and a condition deferred for exactly the cases whose first run reaches the signature
    check through the unrolled P2PKH / P2WPKH path (the construction's kh)."""
    cs = [c for c in RC.load() if c["flags"] == RC.ALL and c["family"] == "key_hash"]
    eng.bcc_set_device_key_hash(1)
    got, st = run(eng, cs, RC.ALL)
    assert got == expected(cs)
    assert st.device_key_hashes == sum(c["kh"] for c in cs) > 9 * 160


# ---- bcc_verify_inputs_batch -------------------------------------------------------------------
def test_verify_inputs_batch_mixed_with_taproot(eng):
    """The 0xE15 cases lifted to (tx, spent outputs, n_in) and mixed with the Taproot goldens under
    0xE15 | TAPROOT (none of these cases spends a native v1 program, so TAPROOT changes nothing for
    them): every answer equals the golden."""
    import mixed_input_cases as M
    ip = ctypes.POINTER(ctypes.c_int)
    eng.bcc_verify_inputs_batch.argtypes = [ctypes.POINTER(B.InputItem), ctypes.c_size_t,
                                            ctypes.c_uint, ip, ip]
    eng.bcc_verify_inputs_batch.restype = ctypes.c_long
    f = M.ALL | M.TAPROOT
    mine = [RC.lifted(c) for c in RC.selection(RC.load()) if c["flags"] == RC.ALL]
    assert not any(M.is_v1(c["spk"]) for c in RC.load())
    tap = [c for c in M.taproot_cases() if c["flags"] == f]
    cases = mine + tap
    random.Random(5).shuffle(cases)
    got = B.verify_inputs_batch(M.items_of(cases), f, library=eng)
    bad = [(c["cls"], tuple(g), c["expected"]) for g, c in zip(got, cases)
           if tuple(g) != tuple(c["expected"])]
    assert not bad, (len(bad), bad[:10])


# ---- the host lane code on the executed checks -------------------------------------------------
def test_host_lane_code_reproduces_every_executed_check(eng):
    """Every distinct (key, signature, sighash) the reference executed in any case, through
    bcc_pubkey_verify_batch with every round on the host lane code: the reference's verdict."""
    seen = {}
    for c in RC.load():
        for k in c["checks"]:
            seen.setdefault((k["pub"], k["sig"], k["sighash"]), k["verdict"])
    ts = [dict(pub=p, sig=s, hash=h) for p, s, h in seen]
    assert len(ts) > 2000 and 0 < sum(seen.values()) < len(ts)
    try:
        eng.bcc_set_host_small_round(1 << 30)
        out = engine_stub.pubkey_verify(eng, ts)
    finally:
        eng.bcc_set_host_small_round(int(os.environ.get("BCC_HOST_SMALL_ROUND", "16")))
    assert list(out) == list(seen.values())
