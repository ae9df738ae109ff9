"""GPU: BIP341 script-path commitment checks through the product C ABI
(bcc_taproot_commit_batch and mi_xonly_tweak_check_tuples: csrc/taproot_commit.hip) against the
reference: every committed case (verdict, error, leaf hash), the wave / workgroup / inversion-group
edges of the batch size, the device list, a fresh random batch checked item by item against
oracle/_ref, and the leaf hash handed on to the tapscript signature check."""
import os
import random
import sys

import pytest

import bitcoinconsensus_amd as B
import commit_cases as C
from oracle_ctypes import Reference, reference_available
from test_taproot_commit_host import check_spends

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 4099]


@pytest.fixture(scope="module")
def golden():
    return C.load_golden()


def as_rows(tuples):
    return [(t["cls"], t["q"], t["parity"], t["p"], t["t"]) for t in tuples]


@pytest.fixture(scope="module")
def pool(golden):
    """A mixed pool (valid, every mutation, wrong control sizes; short scripts) and what each item
    gives when it is the only one of its call: (spends, their results, tuples, their verdicts)."""
    spends, tuples = golden
    sp = [c for c in spends if len(c["script"]) < 300]
    one = []
    for c in sp:
        out, leaves = B.taproot_commit_batch([c], tapleaf=True)
        one.append((out[0], leaves[0]))
    rows = as_rows(tuples)
    tone = [B.xonly_tweak_check_tuples(*C.tuple_rows([r]))[0] for r in rows]
    return sp, one, rows, tone


def test_commit_golden_cases_on_gpu(golden):
    spends, _ = golden
    out, leaves = B.taproot_commit_batch(spends, tapleaf=True)
    check_spends(out, leaves, spends)
    # without the optional leaf output
    assert B.taproot_commit_batch(spends) == out


def test_tweak_golden_tuples_on_gpu(golden):
    _, tuples = golden
    got = B.xonly_tweak_check_tuples(*C.tuple_rows(as_rows(tuples)))
    bad = [(t["cls"], g, t["verdict"]) for t, g in zip(tuples, got) if g != t["verdict"]]
    assert not bad, bad[:10]


def test_single_calls_match_golden(pool, golden):
    """The one-item calls the size tests compare with are themselves the reference's answers."""
    sp, one, rows, tone = pool
    check_spends([o for o, _ in one], [h for _, h in one], sp)
    assert tone == [t["verdict"] for t in golden[1]]


@pytest.mark.parametrize("n", SIZES)
def test_commit_batch_sizes_equal_single_calls(pool, n):
    sp, one, _, _ = pool
    idx = [(7 * i + n) % len(sp) for i in range(n)]  # valid and invalid interleaved
    out, leaves = B.taproot_commit_batch([sp[i] for i in idx], tapleaf=True)
    assert [(o, h) for o, h in zip(out, leaves)] == [one[i] for i in idx]
    assert n < 63 or 0 < sum(o[0] for o in out) < n


@pytest.mark.parametrize("n", SIZES)
def test_tweak_batch_sizes_equal_single_calls(pool, n):
    _, _, rows, tone = pool
    idx = [(5 * i + n) % len(rows) for i in range(n)]
    got = B.xonly_tweak_check_tuples(*C.tuple_rows([rows[i] for i in idx]))
    assert list(got) == [tone[i] for i in idx]


def test_device_list_gives_equal_results(pool):
    """device = -1 over a list naming device 0 three times: contiguous ranges, equal results."""
    sp, one, rows, tone = pool
    n = 3 * 4096 + 5
    idx = [(11 * i) % len(sp) for i in range(n)]
    tidx = [(13 * i) % len(rows) for i in range(n)]
    items, trows = [sp[i] for i in idx], C.tuple_rows([rows[i] for i in tidx])
    B.set_devices([0, 0, 0])
    try:
        out, leaves = B.taproot_commit_batch(items, device=-1, tapleaf=True)
        got = B.xonly_tweak_check_tuples(*trows, device=-1)
    finally:
        B.set_devices([])
    assert [(o, h) for o, h in zip(out, leaves)] == [one[i] for i in idx]
    assert list(got) == [tone[i] for i in tidx]


def test_bad_arguments_verify_nothing():
    import ctypes
    L = B.lib()
    ret, err = (ctypes.c_int * 2)(7, 7), (ctypes.c_int * 2)(7, 7)
    good = B.TaprootCommit(bytes(33), 33, b"", 0, bytes(32))
    for bad in (B.TaprootCommit(None, 33, b"", 0, bytes(32)), B.TaprootCommit(bytes(33), 33, None, 1, bytes(32)),
                B.TaprootCommit(bytes(33), 33, b"", 0, None)):
        arr = (B.TaprootCommit * 2)(good, bad)
        assert L.bcc_taproot_commit_batch(arr, 2, ret, err, None, 0) == -1
        assert list(ret) == [7, 7] and list(err) == [7, 7]
    arr = (B.TaprootCommit * 2)(good, good)
    assert L.bcc_taproot_commit_batch(arr, 2, None, err, None, 0) == -1
    assert L.bcc_taproot_commit_batch(None, 0, None, None, None, 0) == 0
    assert L.mi_xonly_tweak_check_tuples(None, None, None, None, None, 0, 0) == 0
    assert L.mi_xonly_tweak_check_tuples(bytes(32), None, bytes(32), bytes(32), bytes(1), 1, 0) == -1
    # a null script with length 0 is an empty script
    arr = (B.TaprootCommit * 1)(B.TaprootCommit(bytes(33), 33, None, 0, bytes(32)))
    assert L.bcc_taproot_commit_batch(arr, 1, ret, err, None, 0) == 0 and (ret[0], err[0]) == (0, 39)


@pytest.mark.skipif(not reference_available(), reason="oracle/_ref not built")
def test_random_spends_vs_live_reference():
    R = Reference()
    rng = random.Random(0x5C21B7)
    versions = [0xC0, 0xC2, 0xC4, 0xFE, 0x0A, 0x7E]
    lengths = [0, 1, 20, 34, 53, 54, 55, 61, 62, 63, 64, 117, 118, 119, 252, 253, 400]
    depths = [0, 0, 1, 1, 2, 2, 3, 4, 5, 8, 13, 21, 32]
    items = []
    for k in range(3000):
        lv = rng.choice(versions)
        script = b"\x51" if lv == 0xC0 else rng.randbytes(rng.choice(lengths))
        depth = 128 if k % 500 == 0 else rng.choice(depths)
        it = C.make_spend(rng, depth, script, lv)
        r = rng.random()
        if r < 0.35:
            it = C.mutate(rng, it, rng.choice(C.applicable_mutations(it)))
        elif r < 0.4:
            cut = it["control"][: rng.randrange(len(it["control"]) + 1)] + rng.randbytes(rng.randrange(3))
            if cut[:1] != b"\x50":  # the reference would take that control block for an annex
                it = dict(it, control=cut)
        items.append(it)
    out, leaves = B.taproot_commit_batch(items, tapleaf=True)
    bad = []
    for i, it in enumerate(items):
        want = C.ref_spend(R, it)
        if out[i] != want:
            bad.append((i, out[i], want))
        elif want[1] != C.ERR_CONTROL_SIZE and leaves[i] != C.tapleaf(it["control"][0] & 0xFE, it["script"]):
            bad.append((i, "leaf"))
    assert not bad, bad[:10]
    assert 1500 < sum(o[0] for o in out) < 2500
    assert any(o[1] == C.ERR_CONTROL_SIZE for o in out)


@pytest.mark.skipif(not reference_available(), reason="oracle/_ref not built")
def test_random_and_edge_tuples_vs_live_reference():
    T = C.RefTweak(Reference())
    rng = random.Random(0x7EA4C)
    ts = []
    for _ in range(40):  # 40 x 25 edge rows among the random ones
        ts += C.edge_tuples(rng)
    ts += C.walk_tuples(rng, 20000 - len(ts))
    rng.shuffle(ts)
    got = B.xonly_tweak_check_tuples(*C.tuple_rows(ts))
    bad = [(t[0], g) for t, g in zip(ts, got) if g != T.check(*t[1:])]
    assert not bad, bad[:10]
    assert 9000 < sum(got) < 16000


@pytest.mark.skipif(not reference_available(), reason="oracle/_ref not built")
def test_leaf_hash_feeds_the_tapscript_signature_check():
    """End to end: a leaf <key> OP_CHECKSIG committed under a random path; tapleaf_out of the
    commitment entry is the tapleaf_hash32 of bcc_taproot_verify_batch (BCC_SIGVERSION_TAPSCRIPT).
    The signature is over the sighash the reference computes for that leaf hash."""
    import make_taproot_fixtures as G
    R = Reference()
    rng = random.Random(0xE2E)
    for depth in (0, 5):
        sk = rng.randbytes(32)
        _, pk = R.schnorr_sign(sk, bytes(32), bytes(32))
        script = b"\x20" + pk + b"\xac"
        it = C.make_spend(rng, depth, script, 0xC0)
        flipped = C.mutate(rng, it, "script")
        out, leaves = B.taproot_commit_batch([it, flipped], tapleaf=True)
        assert out == [(1, 0), (0, C.ERR_MISMATCH)]
        assert leaves[0] != leaves[1]
        t = G.make_tx(rng, nout=2, long_ok=False)
        nin = rng.randrange(len(t["vin"]))
        G.taproot_input(rng, t, nin)
        t["spent"][nin] = (t["spent"][nin][0], b"\x51\x20" + it["program"])
        t["wit"][nin] = [bytes(64), it["script"], it["control"]]
        tx, spent = G.tx_bytes(t), G.ser_outs(t["spent"])
        _, _, h = R.taproot_check(tx, spent, nin, bytes(64), bytes(32), B.SIGVERSION_TAPSCRIPT, None,
                                  leaves[0], 0xFFFFFFFF)
        sig, pk2 = R.schnorr_sign(sk, h, rng.randbytes(32))
        assert pk2 == pk
        chk = dict(tx=tx, spent=spent, nin=nin, sig=sig, pk=pk, sigversion=B.SIGVERSION_TAPSCRIPT,
                   tapleaf=leaves[0], codesep=0xFFFFFFFF)
        res = B.taproot_verify_batch([chk, dict(chk, tapleaf=leaves[1])])
        assert res == [(1, 0), (0, B.SCRIPT_ERR_SCHNORR_SIG)]
