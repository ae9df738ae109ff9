"""GPU: the engine's second and later device rounds through librbc_amd.so, on the verdict-dependent
spends of tests/golden/rerun_cases.json.gz (tests/rerun_cases.py; expected values recorded from the
reference, rounds_min from the construction): one-item batches, whole calls, a small round staged
on a DeviceBatch that just ran a large one (key-hash conditions, pre-uploaded rows, the verdict
buffer and the DER rows of round 1 must not reach round 2), every switch that "never changes
results" combined with a re-run, key_hash_kernel's 20-byte comparison one bit at a time, two caller
threads, and bcc_verify_inputs_batch.  conftest.py forbids a host fallback; nothing is injected.
CPU twin: test_rerun_host.py."""
import ctypes
import os
import random
import threading

import pytest

import bitcoinconsensus_amd as B
import rerun_cases as RC

pytestmark = pytest.mark.gpu

PIPELINE_CHUNK_DEFAULT = 500_000  # engine.cpp g_pipeline_chunk
HOST_SMALL_ROUND = int(os.environ.get("BCC_HOST_SMALL_ROUND", "16"))  # conftest.py: 0
PRE_UPLOAD = int(os.environ.get("BCC_PRE_UPLOAD", "1") or 0) != 0  # engine.cpp g_pre_upload


class Call:
    """A verify_batch call staged once (items of one transaction share its buffer)."""

    def __init__(self, cases, flags=RC.ALL):
        self.cases, self.flags, self.n = cases, flags, len(cases)
        self.arr, self.keep = B._batch_items([RC.item(c) for c in cases])
        self.expected = [(c["ret"], c["err"]) for c in cases]

    def run(self):
        ret = (ctypes.c_int * self.n)()
        err = (ctypes.c_int * self.n)()
        rc = B.lib().bitcoinconsensus_verify_batch(self.arr, self.n, self.flags, ret, err)
        got = list(zip(ret, err))
        assert rc == sum(r for r, _ in got)
        return got, B.last_batch_stats()

    def check(self, got):
        bad = [(c["name"], g, e) for c, g, e in zip(self.cases, got, self.expected) if g != e]
        assert not bad, (len(bad), bad[:10])


@pytest.fixture(autouse=True)
def every_round_on_the_device():
    B.set_host_small_round(0)
    yield
    B.set_host_small_round(HOST_SMALL_ROUND)


def test_one_item_batches():
    """The cases built for a re-run and every 10th other case, each alone."""
    bad, hist = [], {}
    for c in RC.selection(RC.load()):
        call = Call([c], c["flags"])
        got, st = call.run()
        hist[st["rounds"]] = hist.get(st["rounds"], 0) + 1
        # a CHECKMULTISIG re-run is offered every candidate pair: never more than one extra round
        most = 2 if c["family"] == "multisig" else 4
        if got != call.expected or not c["rounds_min"] <= st["rounds"] <= most:
            bad.append((c["name"], hex(c["flags"]), got, call.expected, st["rounds"], c["rounds_min"]))
    print("rounds histogram of the one-item batches:", sorted(hist.items()))
    assert not bad, (len(bad), bad[:10])
    assert hist[2] >= 200 and hist[3] >= 40 and hist[4] >= 8


@pytest.mark.parametrize("flags", RC.FLAG_SETS)
def test_all_cases_in_one_call(flags):
    cs = [c for c in RC.load() if c["flags"] == flags]
    for seed in (None, 1):
        order = list(cs)
        if seed is not None:
            random.Random(seed).shuffle(order)
        call = Call(order, flags)
        got, st = call.run()
        call.check(got)
        assert st["rounds"] >= 4


# ---- a small round after a large one -----------------------------------------------------------
_scattered = None


def scattered():
    """About 20,000 all-valid one-round items (the file's, tiled) with every case of two or more
    rounds scattered among them, and the plain run's answers: round 1 is large, rounds 2-4 small."""
    global _scattered
    if _scattered is None:
        cs = [c for c in RC.load() if c["flags"] == RC.ALL]
        valid = [c for c in cs if c["ret"] == 1 and c["rounds_min"] == 1]
        rerun = [c for c in cs if c["rounds_min"] >= 2]
        assert len(valid) >= 100 and len(rerun) >= 100
        items = [valid[i % len(valid)] for i in range(20000)]
        rng = random.Random(20)
        for c in rerun:
            items.insert(rng.randrange(len(items) + 1), c)
        call = Call(items)
        plain, st = call.run()
        _scattered = (call, plain, st)
    return _scattered


def test_small_rounds_after_a_large_one():
    call, plain, st = scattered()
    call.check(plain)
    assert st["rounds"] >= 4 and st["host_rounds"] == 0
    assert st["tuples"] > 20000 and st["device_key_hashes"] > 0


SETTINGS = {
    # at least 9 chunks, whose re-run rounds stage beside the next chunk's first round
    "pipeline_chunk_2048": (lambda: B.set_pipeline_chunk(2048),
                            lambda: B.set_pipeline_chunk(PIPELINE_CHUNK_DEFAULT)),
    "devices_0_0": (lambda: B.set_devices([0, 0]), lambda: B.set_devices([])),
    "direct_upload_off": (lambda: B.set_direct_upload(0), lambda: B.set_direct_upload(1)),
    "pre_upload_off_pipelined": (
        lambda: (B.set_pipeline_chunk(2048), B.set_pre_upload(0)),
        lambda: (B.set_pipeline_chunk(PIPELINE_CHUNK_DEFAULT), B.set_pre_upload(PRE_UPLOAD))),
    "early_q_off": (lambda: B.set_early_q(0), lambda: B.set_early_q(1)),
    "early_q_on": (lambda: B.set_early_q(1), lambda: B.set_early_q(1)),
    "host_chain_blocks_0": (lambda: B.set_host_chain_blocks(0),
                            lambda: B.set_host_chain_blocks(B.HOST_CHAIN_BLOCKS_DEFAULT)),
    "device_key_hash_off": (lambda: B.set_device_key_hash(0), lambda: B.set_device_key_hash(1)),
}


@pytest.mark.parametrize("name", list(SETTINGS))
def test_settings_never_change_a_rerun(name):
    call, plain, _ = scattered()
    on, off = SETTINGS[name]
    try:
        on()
        got, st = call.run()
    finally:
        off()
    assert got == plain
    assert st["rounds"] >= 4
    if name == "early_q_on":
        assert st["early_mapped"] > 0
    if name == "early_q_off":
        assert st["early_rows"] == 0 and st["early_mapped"] == 0
    if name == "devices_0_0":
        assert st["devices"] == 2
    if name == "device_key_hash_off":
        assert st["device_key_hashes"] == 0
    assert st["host_rounds"] == 0


def test_production_shape_small_later_rounds_on_the_host():
    """bcc_set_host_small_round(16) with re-run rounds of at most 16 checks, as in production: the
    same large first round with only a few verdict-dependent spends among it (the four-round
    ladders, a CHECKSIG NOT IF and the OP_CODESEPARATOR pair: one new check per re-run each).  The
    first round runs on the GPU, the later ones in the host lane code, with the plain answers."""
    call, _, _ = scattered()
    few = [c for c in call.cases if c["rounds_min"] == 4 and c["name"].startswith("ladder:4:")
           and c["name"].endswith(":compressed")]
    few += [c for c in call.cases if c["name"] in ("notif:10:bare", "codesep:first_valid=0")]
    assert len(few) == 6
    items = [c for c in call.cases if c["rounds_min"] < 2]
    rng = random.Random(21)
    for c in few:
        items.insert(rng.randrange(len(items) + 1), c)
    sparse = Call(items)
    plain, st0 = sparse.run()
    sparse.check(plain)
    assert st0["rounds"] == 4 and st0["host_rounds"] == 0
    try:
        B.set_host_small_round(16)
        got, st = sparse.run()
    finally:
        B.set_host_small_round(0)
    assert got == plain
    assert st["rounds"] == 4 and 0 < st["host_rounds"] < st["rounds"]


def test_key_hash_near_misses():
    """key_hash_kernel alone decides these: a valid signature under a program one bit away from
    HASH160(key), for every bit, kind and key form.  A comparison that skipped a word or a byte
    would accept one of them."""
    cs = [c for c in RC.load() if c["flags"] == RC.ALL and c["family"] == "key_hash"]
    call = Call(cs)
    B.set_device_key_hash(1)
    got, st = call.run()
    call.check(got)
    assert st["device_key_hashes"] == sum(c["kh"] for c in cs)
    for kind in RC.KH_KINDS:
        for form in RC.KEY_FORMS:
            sweep = {int(c["name"].split(":")[3]): g for c, g in zip(cs, got)
                     if c["name"].startswith("%s:%s:sweep:" % (kind, form))}
            assert sorted(sweep) == list(range(160))
            assert [b for b, g in sweep.items() if g[0] != 0] == [], (kind, form)


def test_two_caller_threads():
    call, plain, _ = scattered()
    out = [None, None]

    def work(k):
        try:
            out[k] = call.run()[0]
        finally:
            B.release_thread_state()

    ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert out[0] == plain and out[1] == plain


def test_verify_inputs_batch_mixed_with_taproot():
    """The 0xE15 cases lifted to (tx, spent outputs, n_in), mixed with the Taproot goldens under
    0xE15 | TAPROOT: every answer equals the golden."""
    import mixed_input_cases as M
    f = M.ALL | M.TAPROOT
    cases = [RC.lifted(c) for c in RC.load() if c["flags"] == RC.ALL]
    cases += [c for c in M.taproot_cases() if c["flags"] == f]
    random.Random(5).shuffle(cases)
    got = B.verify_inputs_batch(M.items_of(cases), f)
    bad = [(c["cls"], tuple(g), c["expected"]) for g, c in zip(got, cases)
           if tuple(g) != tuple(c["expected"])]
    assert not bad, (len(bad), bad[:10])
