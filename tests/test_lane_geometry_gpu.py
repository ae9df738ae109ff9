"""GPU: adversarial rows INSIDE the inversion chains of the signature stage.

K_inv (batch_sinv_kernel) and K_tfin (twist_fin_kernel) share one inversion among the lanes
t, t + T, ... of a thread; below cus * 256 rows T equals the row count and no row shares anything.
The batches of tests/lane_geometry.py are large enough to form chains (up to 16 lanes) and put every
class whose lane leaves the normal path at chosen positions of chosen chains.  Every row of every
batch is compared with its golden verdict (the reference's), and the batch's sum with the expected
sum.  Before running, each test asserts through the library's launch-shape export
(bcc_debug_launch_shape: the launchers' own helpers) that its batch takes the shape it was built
for -- on any CU count.  Expected verdicts never come from the export."""
import ctypes
import threading

import numpy as np
import pytest

import lane_geometry as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import bitcoinconsensus_amd as B
    s = B.debug_launch_shape(1)
    assert s["cus"] == B.blib().mi_device_cus(0) > 0
    assert s["inv_per_thread"] == s["fin_per_thread"] == G.PER_THREAD
    return dict(cus=s["cus"], wg=s["ladder_wg"], R=s["round_lanes"])


def _ecdsa(tab, idx):
    import bitcoinconsensus_amd as B
    return B.ecdsa_verify_tuples(*(tab.pack(idx, k) for k in ("pub65", "hash", "r32", "s32")))


def _schnorr(tab, idx):
    import bitcoinconsensus_amd as B
    return B.schnorr_verify_tuples(*(tab.pack(idx, k) for k in ("sig", "msg", "pub")))


RUN = {"ecdsa": _ecdsa, "schnorr": _schnorr}


def _check(tab, idx, got, chunks):
    """Every row against its golden verdict; chunks = [(base, cnt, T)] for the failure report."""
    assert len(got) == len(idx)
    bad = []
    for base, cnt, T in chunks:
        bad += G.mismatches(tab, idx[base:base + cnt], got[base:base + cnt], T, base, 20 - len(bad))
    assert not bad, ("(class, lane, chain, position, chain length, got, expected)", bad)
    assert sum(got) == int(G.expected(tab, idx).sum())


def _assert_one_chunk_shape(n, dev, T):
    """The batch runs as one chunk whose K_inv and K_tfin threads are T, in the mode the sizes'
    rule gives (for the chain batches: never the latency mode)."""
    import bitcoinconsensus_amd as B
    s = B.debug_launch_shape(n)
    assert s["chunks"] == 1 and s["chunk_stride"] >= n, s
    assert s["inv_threads"] == s["fin_threads_first"] == s["fin_threads_last"] == T, (s, T)
    assert (s["mode"], s["split_at"]) == G.size_shape(n, dev["cus"], dev["R"]), s
    return s


@pytest.fixture(scope="module")
def full_ecdsa(dev):
    """chains_full for ECDSA and its verdicts through the tuple ABI (shared by two tests)."""
    tab = G.ecdsa_table()
    idx, rec = G.chains_full(dev["cus"], "ecdsa")
    G.assert_full_coverage(rec, "ecdsa")
    s = _assert_one_chunk_shape(rec["n"], dev, rec["T"])
    assert rec["T"] == dev["cus"] * 256 and -(-rec["n"] // rec["T"]) == 16 and s["mode"] != "latency"
    return tab, idx, rec, _ecdsa(tab, idx)


def test_chains_full_ecdsa_tuples(full_ecdsa):
    """Chains of 16 (the last 37 of 15): every non-normal class alone among valid rows at the
    first, second, middle and last positions, chains that never multiply, chains with one valid
    row at each position, adjacent doublings; raw r32 / s32 >= n among the classes."""
    tab, idx, rec, got = full_ecdsa
    _check(tab, idx, got, [(0, rec["n"], rec["T"])])


def test_chains_full_ecdsa_blob_abi(full_ecdsa):
    """The same lanes through bcc_pubkey_verify_batch (lax DER on the device in front of the same
    kernels).  The raw out-of-range rows have no DER form: their lanes hold a valid row here.  A
    call of this size runs as pipelined rounds of its own sizes, so its chains are the rounds'
    (still several lanes each); the verdicts must be the golden ones and, on the shared rows,
    identical to the tuple call's."""
    import bitcoinconsensus_amd as B
    tab, idx, rec, first = full_ecdsa
    idx2 = idx.copy()
    raw = tab.raw[idx]
    assert raw.sum() >= len(G.RAW_CLASSES) * G.RAW_PER_CLASS
    idx2[raw] = tab.filler[0]
    pb, po = tab.blob(idx2, "pub", "publen")
    sb, so = tab.blob(idx2, "sig", "siglen")
    msg = np.ascontiguousarray(tab.cols["hash"][idx2])
    n = len(idx2)
    L = ctypes.CDLL(B.lib()._name)  # own handle: argtypes of its own
    u64p, vp = ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p
    f = L.bcc_pubkey_verify_batch
    f.argtypes = [vp, u64p, vp, vp, u64p, vp, ctypes.c_size_t, ctypes.c_int]
    out = np.zeros(n, np.uint8)
    assert f(pb.ctypes.data, po.ctypes.data_as(u64p), msg.ctypes.data, sb.ctypes.data,
             so.ctypes.data_as(u64p), out.ctypes.data, n, 0) == 0
    _check(tab, idx2, out.tobytes(), [(0, n, rec["T"])])
    same = np.frombuffer(first, np.uint8)[~raw] == out[~raw]
    assert same.all(), np.flatnonzero(~raw)[~same][:20]


def test_chains_full_schnorr_tuples(dev):
    """BIP340 in chains of 16: s = +-e d (x(A) == x(B): infinity and the doubling sum), s = 0,
    r >= p, keys off the curve or >= p, s >= n, the all-zero row."""
    import bitcoinconsensus_amd as B
    tab = G.schnorr_table()
    idx, rec = G.chains_full(dev["cus"], "schnorr")
    G.assert_full_coverage(rec, "schnorr")
    s = B.debug_launch_shape(rec["n"])
    assert s["chunks"] == 1 and s["fin_threads_first"] == s["fin_threads_last"] == rec["T"], s
    assert -(-rec["n"] // rec["T"]) == 16
    _check(tab, idx, _schnorr(tab, idx), [(0, rec["n"], rec["T"])])


@pytest.mark.parametrize("kind", ["ecdsa", "schnorr"])
def test_chains_chunked(dev, kind):
    """Three chunks with chains of two (19 of them in the short last chunk), the non-normal rows
    at both positions right after each chunk's base: once as one chunk (chains of five and six)
    and once chunked; golden verdicts both times, byte-identical outputs."""
    import bitcoinconsensus_amd as B
    tab = G.table(kind)
    cus = dev["cus"]
    idx, rec = G.chains_chunked(cus, kind)
    G.assert_chunked_coverage(rec, kind)
    n, C, chunks = G.chunked_shape(cus)
    T1 = G.threads(n, cus)
    s = B.debug_launch_shape(n)
    assert s["chunks"] == 1 and s["fin_threads_first"] == T1 == cus * 256 and s["inv_threads"] == T1, s
    one = RUN[kind](tab, idx)
    B.set_chunk_lanes(C)
    try:
        s = B.debug_launch_shape(n)
        assert (s["mode"], s["chunk_stride"], s["chunks"]) == ("chunked", C, 3), s
        assert s["fin_threads_first"] == rec["chunks"][0]["T"] == cus * 256, s
        assert s["fin_threads_last"] == rec["chunks"][2]["T"] == cus * 256, s
        assert rec["chunks"][2]["cnt"] - s["fin_threads_last"] == 19
        assert s["inv_threads"] == T1  # K_inv runs over the whole batch
        three = RUN[kind](tab, idx)
    finally:
        B.set_chunk_lanes(0)
    _check(tab, idx, one, [(0, n, T1)])
    _check(tab, idx, three, [(c["base"], c["cnt"], c["T"]) for c in rec["chunks"]])
    assert three == one


@pytest.mark.parametrize("which", range(len(G.SIZE_NAMES)), ids=G.SIZE_NAMES)
def test_sizes(dev, which):
    """Every size at which the launch shape changes (lane_geometry.sizes): the latency mode's
    bound, the first chain of two, a K_keyq tail launch of one lane, two whole residency rounds.
    ECDSA at every size, BIP340 up to 2 * cus * 256 + 1; around R the ECDSA batch also runs in a
    second thread (its scratch, second stream and events are created there) beside a small batch
    in this one."""
    import bitcoinconsensus_amd as B
    cus, wg, R = dev["cus"], dev["wg"], dev["R"]
    ns = G.sizes(cus, wg, R)
    assert len(ns) == len(G.SIZE_NAMES)
    n = ns[which]
    tab = G.ecdsa_table()
    idx, rec = G.size_batch(n, cus, wg, R, "ecdsa")
    T = G.threads(n, cus)
    s = _assert_one_chunk_shape(n, dev, T)
    assert s["split_at"] == rec["A"]
    got = _ecdsa(tab, idx)
    _check(tab, idx, got, [(0, n, T)])
    if n <= 2 * cus * 256 + 1:
        stab = G.schnorr_table()
        sidx, _ = G.size_batch(n, cus, wg, R, "schnorr")
        ss = B.debug_launch_shape(n)
        assert ss["chunks"] == 1 and ss["fin_threads_first"] == T
        _check(stab, sidx, _schnorr(stab, sidx), [(0, n, T)])
    if n in (R - 1, R, R + 1):
        small, _ = G.size_batch(1000, cus, wg, R, "ecdsa")
        res = {}

        def work():
            try:
                res["big"] = _ecdsa(tab, idx)
            except Exception as e:  # reported below, on the main thread
                res["error"] = e

        th = threading.Thread(target=work)
        th.start()
        res["small"] = [_ecdsa(tab, small) for _ in range(3)]
        th.join()
        assert "error" not in res, res["error"]
        _check(tab, idx, res["big"], [(0, n, T)])
        assert res["big"] == got
        for v in res["small"]:
            _check(tab, small, v, [(0, 1000, G.threads(1000, cus))])


@pytest.mark.parametrize("mirror", [False, True])
def test_decided_chain_tweak_rows(mirror):
    """tweak_fin_kernel with T = 2 over 32 rows: one chain holds only rows tweak_add_lane decided
    (its product stays 1), the other only valid rows."""
    import bitcoinconsensus_amd as B
    rows, rec = G.decided_chain(mirror)
    assert B.debug_commit_fin_threads(rec["n"]) == rec["T"] == 2
    got = B.xonly_tweak_check_tuples(b"".join(t["q"] for t in rows), bytes(t["parity"] for t in rows),
                                     b"".join(t["p"] for t in rows), b"".join(t["t"] for t in rows))
    bad = [(t["cls"], i, *G.chain_of(i, 32, 2), got[i], t["verdict"]) for i, t in enumerate(rows)
           if got[i] != t["verdict"]]
    assert not bad, bad
    assert sum(got) == sum(t["verdict"] for t in rows)
