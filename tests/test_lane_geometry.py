"""CPU: the placed batches of tests/lane_geometry.py hold what they promise (the coverage
conditions, for three CU counts), chain_of partitions a chunk's lanes, expected verdicts are the
golden ones, and the new rows (raw r32 / s32 >= n, BIP340 s = +-e d) have CPU twins on both host
builds of the lane code.  The launch-shape export of the library needs no GPU either."""
import numpy as np
import pytest

import lane_geometry as G
from fixtures import pub_to_tuple
from test_lane_host import arith, lane  # noqa: F401  (the two host builds of the lane code)

CUS = (64, 256, 304)
WG = 256
KINDS = ("ecdsa", "schnorr")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cus", CUS)
def test_chains_full_coverage(cus, kind):
    tab = G.table(kind)
    idx, rec = G.chains_full(cus, kind)
    assert len(idx) == rec["n"] == 16 * cus * 256 - 37 and rec["T"] == cus * 256
    G.assert_full_coverage(rec, kind)
    # the expected verdicts are the golden verdicts of the indexed rows; the filler rows all verify,
    # so the batch's sum is the fixture rows' sum plus the filler count
    exp = G.expected(tab, idx)
    assert np.array_equal(exp, tab.verdict[idx])
    is_fill = np.isin(idx, tab.filler)
    assert exp[is_fill].all() and int(exp.sum()) == int(is_fill.sum()) + int(exp[~is_fill].sum())
    # ragged: exactly the last 37 chains have 15 members
    lengths = [G.chain_of(t, rec["n"], rec["T"])[2] for t in range(rec["T"] - 40, rec["T"])]
    assert lengths == [16] * 3 + [15] * 37


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cus", CUS)
def test_chains_chunked_coverage(cus, kind):
    tab = G.table(kind)
    idx, rec = G.chains_chunked(cus, kind)
    n, C, chunks = G.chunked_shape(cus)
    assert len(idx) == n == 5 * cus * 256 + 19 and C == 2 * cus * 256 and len(chunks) == 3
    assert [c["cnt"] for c in rec["chunks"]] == [C, C, cus * 256 + 19]
    G.assert_chunked_coverage(rec, kind)
    for c in rec["chunks"]:  # chains of two everywhere in the first chunks, 19 of them in the last
        lens = [G.chain_of(i, c["cnt"], c["T"])[2] for i in (0, c["two"] - 1, c["two"], c["T"] - 1)]
        assert lens == ([2, 2, 2, 2] if c["two"] == c["T"] else [2, 2, 1, 1])
    assert np.array_equal(G.expected(tab, idx), tab.verdict[idx])


@pytest.mark.parametrize("cus", CUS)
def test_sizes_and_their_batches(cus):
    R = cus * 1024
    ns = G.sizes(cus, WG, R)
    assert len(ns) == len(set(ns)) == 24 and ns == sorted(ns)
    assert {1, cus * 128, cus * 128 + 1, cus * 256 + 1, R + 1, 2 * R, 2 * R + 1} <= set(ns)
    modes = {n: G.size_shape(n, cus, R) for n in ns}
    assert modes[cus * 128] == ("latency", 0) and modes[cus * 128 + 1] == ("one_launch", 0)
    assert modes[R] == ("one_launch", 0) and modes[R + 1] == ("split", R)
    assert modes[2 * R] == ("one_launch", 0) and modes[2 * R + 1] == ("split", 2 * R)
    for kind in KINDS:
        tab = G.table(kind)
        for n in ns:
            idx, rec = G.size_batch(n, cus, WG, R, kind)
            assert len(idx) == n and np.array_equal(G.expected(tab, idx), tab.verdict[idx])
            at = {name: (lane_, cls) for name, lane_, cls in rec["placed"] if cls == G.DOUBLING[kind]}
            assert at["last"][0] == n - 1
            w0 = (n - 1) // WG * WG  # the last workgroup's first lane, unless the last lanes took it
            if w0 < n - 2:
                assert at["last_wg"][0] == w0
            if n >= 2:
                assert any(c == G.REJECTED[kind] for _, _, c in rec["placed"])
            if rec["A"]:  # the tail launch's first lane (at R + 1 it is the last lane as well)
                assert rec["A"] == n // R * R and tab.cls_name(idx[rec["A"]]) == G.DOUBLING[kind]
            if n >= len(tab) + 8:  # the whole table recurs
                assert len(set(idx.tolist())) == len(tab)


@pytest.mark.parametrize("cus", CUS)
def test_chain_of_partitions_the_lanes(cus):
    """chain_of against the definition: thread t owns lanes t, t + T, ... below cnt."""
    R = cus * 1024
    for cnt in G.sizes(cus, WG, R)[:17] + [16 * cus * 256 - 37]:
        T = G.threads(cnt, cus)
        assert T == max((cnt + 15) // 16, min(cnt, cus * 256))
        lanes = np.arange(cnt)
        owner, pos = lanes % T, lanes // T
        length = np.bincount(owner, minlength=T)
        assert length.sum() == cnt and length.max() <= 16 and length.min() >= 1
        seen = np.zeros(cnt, bool)
        for t in {0, 1, T // 2, T - 1} | {int(x) for x in np.random.default_rng(cnt).integers(T, size=8)}:
            own = list(range(t, cnt, T))
            assert [G.chain_of(i, cnt, T) for i in own] == [(t, p, len(own)) for p in range(len(own))]
            seen[own] = True
        # every lane is in exactly one chain, at one position
        assert len(set(zip(owner.tolist(), pos.tolist()))) == cnt
        for i in (0, cnt - 1, cnt // 2):
            t, p, ln = G.chain_of(i, cnt, T)
            assert (t, p, ln) == (int(owner[i]), int(pos[i]), int(length[t])) and t + p * T == i


def test_decided_chain():
    for mirror in (False, True):
        rows, rec = G.decided_chain(mirror)
        assert rec["n"] == 32 and rec["T"] == 2 == -(-32 // 16)
        assert rec["chains"] == {1 if mirror else 0} and len(rec["decided_lanes"]) == 16
        assert {"t_zero_par0", "p_off_curve", "parity_2", "infinity_q0", "p_eq_prime"} <= \
            {c[4:] if c.startswith("mix_") else c for c in rec["classes"]}
        assert all(rows[i]["verdict"] == 1 for i in range(32) if i not in rec["decided_lanes"])
        assert sum(t["verdict"] for t in rows) >= 17  # t_zero_par0 is decided and true


def test_raw_rows_are_out_of_range():
    tab = G.ecdsa_table()
    for cls, (rv, sv) in G.RAW_CLASSES.items():
        rows = tab.rows_of(cls)
        assert len(rows) == G.RAW_PER_CLASS and not tab.verdict[rows].any() and tab.raw[rows].all()
        for i in rows:
            r, s = (int.from_bytes(tab.cols[k][i].tobytes(), "big") for k in ("r32", "s32"))
            assert r >= G.N or s >= G.N
            assert (rv is None or r == rv) and (sv is None or s == sv)
            assert tab.cols["siglen"][i] == 0  # never goes to a DER entry


@pytest.mark.parametrize("fn", ["lane_verify_twist", "lane_verify_twist_host"])
def test_placed_rows_on_the_host_lane_builds_ecdsa(arith, fn):  # noqa: F811
    """A few hundred lanes of chains_full (every raw out-of-range row among them) through both
    forms of the lane code on both host builds: the expected verdict of each."""
    tab = G.ecdsa_table()
    idx, _ = G.chains_full(64, "ecdsa")
    rng = np.random.default_rng(7)
    lanes = np.concatenate([np.flatnonzero(tab.raw[idx]), rng.choice(len(idx), 300, replace=False)])
    assert tab.raw[idx[lanes]].sum() >= len(G.RAW_CLASSES) * G.RAW_PER_CLASS
    f, bad = getattr(arith, fn), []
    for i in lanes:
        row = idx[i]
        p65 = tab.cols["pub65"][row].tobytes()
        got = f(p65[0], p65[1:33], p65[33:], tab.cols["r32"][row].tobytes(),
                tab.cols["s32"][row].tobytes(), tab.cols["hash"][row].tobytes())
        if got != tab.verdict[row]:
            bad.append((tab.cls_name(row), int(i), got, int(tab.verdict[row])))
    assert not bad, (len(bad), bad[:10])


def test_placed_rows_on_the_host_lane_builds_schnorr(arith):  # noqa: F811
    tab = G.schnorr_table()
    idx, _ = G.chains_full(64, "schnorr")
    rng = np.random.default_rng(8)
    new = np.flatnonzero(np.isin(tab.cls[idx], [tab.classes.index(c) for c in
                                                ("s_eq_ed", "s_eq_minus_ed", "s_eq_ed/nb",
                                                 "s_eq_minus_ed/nb")]))
    lanes = np.concatenate([new[:300], rng.choice(len(idx), 200, replace=False)])
    bad = []
    for i in lanes:
        row = idx[i]
        got = arith.lane_schnorr_verify_twist(tab.cols["sig"][row].tobytes(), tab.cols["msg"][row].tobytes(),
                                              tab.cols["pub"][row].tobytes())
        if got != tab.verdict[row]:
            bad.append((tab.cls_name(row), int(i), got, int(tab.verdict[row])))
    assert not bad, (len(bad), bad[:10])


def test_launch_shape_export_matches_the_stated_formula():
    """bcc_debug_launch_shape (no GPU: the CU count is given) against the T formula and the routing
    rules as the design states them, at every size edge and at the two chain batches."""
    import bitcoinconsensus_amd as B
    for cus in CUS:
        s0 = B.debug_launch_shape(1, cus)
        R, wg = s0["round_lanes"], s0["ladder_wg"]
        assert s0["cus"] == cus and R % wg == 0 and s0["inv_per_thread"] == s0["fin_per_thread"] == 16
        for n in G.sizes(cus, wg, R) + [16 * cus * 256 - 37]:
            s = B.debug_launch_shape(n, cus)
            assert (s["mode"], s["split_at"]) == G.size_shape(n, cus, R), (cus, n, s)
            assert s["inv_threads"] == s["fin_threads_first"] == s["fin_threads_last"] == G.threads(n, cus)
            assert s["chunks"] == 1 and s["chunk_stride"] == (n + 255) // 256 * 256
        n, C, chunks = G.chunked_shape(cus)
        B.set_chunk_lanes(C)
        try:
            s = B.debug_launch_shape(n, cus)
        finally:
            B.set_chunk_lanes(0)
        assert (s["mode"], s["chunk_stride"], s["chunks"]) == ("chunked", C, 3)
        assert s["fin_threads_first"] == G.threads(chunks[0][1], cus) == cus * 256
        assert s["fin_threads_last"] == G.threads(chunks[-1][1], cus) == cus * 256
    assert B.debug_commit_fin_threads(32) == 2
