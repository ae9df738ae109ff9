"""Batches with rows PLACED in the signature stage's inversion chains (no GPU needed to build them).

The ECDSA and BIP340 kernels share one field inversion among the lanes a thread walks: thread t of
K_inv (batch_sinv_kernel) and of K_tfin (twist_fin_kernel) owns lanes t, t + T, t + 2 T, ... below
the chunk's lane count, with

    T = max(ceil(cnt / 16), min(cnt, cus * 256))

so chains of two start above cus * 256 rows and full chains of 16 need about 16 * cus * 256.  What
such a design can get wrong is a row poisoning the verdicts of the other rows of its chain; the
builders here put every golden class whose lane leaves the normal path (TW_EXCEPT, TW_REJECT, a
sanitised s) at chosen positions of chosen chains, among valid rows.

Rows live in tables of numpy arrays; a batch is an index vector into a table, and its bytes come
from fancy indexing.  Every builder returns (index vector, record); the record holds coverage facts
that are computed from the finished index vector.  Expected verdicts are the golden verdicts of the
indexed rows (the reference's), never anything a kernel or the library reports."""
import numpy as np

from fixtures import (bip340_vectors, ecdsa_tuples, pub_to_tuple, schnorr_exceptional, schnorr_tuples,
                      structured_scalars)

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
PER_THREAD = 16

# Raw (r32, s32) values no DER signature yields (the lax parser maps overflow to 0): the reference
# has no scalar for them, CPubKey::Verify sees (0, 0) and fails.  Tuple ABI only.
RAW_CLASSES = {"raw_s_eq_n": (None, N), "raw_s_n_plus_1": (None, N + 1), "raw_s_max": (None, 2**256 - 1),
               "raw_r_eq_n": (N, None), "raw_r_max": (2**256 - 1, None),
               "raw_r_s_ge_n": (2**256 - 1, N + 1)}
RAW_PER_CLASS = 8

# Classes whose lane is TW_EXCEPT or TW_REJECT or has its s sanitised, the exceptional sums first.
NON_NORMAL = {
    "ecdsa": ("a_equals_b", "a_equals_minus_b_s1", "r_infinity", "structured", "u1_zero", "s_zero",
              "r_zero", "x_no_sqrt", "x_ge_p", "bad_header", "u_wrong_y") + tuple(RAW_CLASSES),
    "schnorr": ("s_eq_ed", "s_eq_minus_ed", "s_zero", "r_ge_p", "pub_off_curve", "pub_ge_p", "s_ge_n",
                "zero_everything"),
}
DOUBLING = {"ecdsa": "a_equals_b", "schnorr": "s_eq_minus_ed"}  # valid / invalid rows that double
REJECTED = {"ecdsa": "s_zero", "schnorr": "s_ge_n"}


class Table:
    """Rows as arrays: cols[name] is (rows, width) uint8 (or (rows,) for lengths); cls indexes
    `classes`; verdict is the golden verdict; non_normal marks NON_NORMAL rows; filler lists the
    valid rows batches are filled with."""

    def __init__(self, kind, cols, cls_names, verdict, filler_classes):
        self.kind, self.cols = kind, cols
        self.classes = sorted(set(cls_names))
        lut = {c: i for i, c in enumerate(self.classes)}
        self.cls = np.array([lut[c] for c in cls_names], np.int32)
        self.verdict = np.asarray(verdict, np.uint8)
        self.non_normal_classes = NON_NORMAL[kind]
        missing = [c for c in self.non_normal_classes if c not in lut]
        assert not missing, missing
        self.non_normal = np.isin(self.cls, [lut[c] for c in self.non_normal_classes])
        self.raw = np.isin(self.cls, [lut[c] for c in RAW_CLASSES if c in lut])
        self.filler = np.flatnonzero(np.isin(self.cls, [lut[c] for c in filler_classes])
                                     & (self.verdict == 1))
        self.good = (self.verdict == 1) & ~self.non_normal  # a valid row on the normal path
        self._rows = {c: np.flatnonzero(self.cls == i) for c, i in lut.items()}

    def __len__(self):
        return len(self.verdict)

    def rows_of(self, cls):
        return self._rows[cls]

    def cls_name(self, row):
        return self.classes[self.cls[row]]

    def pack(self, idx, col):
        return np.ascontiguousarray(self.cols[col][idx]).tobytes()

    def blob(self, idx, col, lencol):
        """(blob, uint64 offsets) of a variable-length column for the blob ABI."""
        lens = self.cols[lencol][idx].astype(np.uint64)
        off = np.zeros(len(idx) + 1, np.uint64)
        np.cumsum(lens, out=off[1:])
        rows = self.cols[col][idx]
        keep = np.arange(rows.shape[1], dtype=np.uint64)[None, :] < lens[:, None]
        return np.concatenate([rows[keep], np.zeros(1, np.uint8)]), off


def _rows2d(items, width):
    a = np.zeros((len(items), width), np.uint8)
    for i, b in enumerate(items):
        a[i, :len(b)] = np.frombuffer(b, np.uint8)
    return a


_tables = {}


def ecdsa_table():
    """structured_scalars()["ecdsa"] and ecdsa_tuples(), packed as test_structured_scalars_gpu.py
    packs them (the checker-side lax DER parse for rows without r32 / s32), plus the raw
    out-of-range rows.  Columns: pub65, hash, r32, s32, sig + siglen (DER), pub + publen."""
    if "ecdsa" in _tables:
        return _tables["ecdsa"]
    from oracle_ctypes import Oracle
    O = Oracle()
    rows = []
    for t in structured_scalars()["ecdsa"] + ecdsa_tuples():
        tag, x, y = pub_to_tuple(t["pub"])
        if "r32" in t:
            r, s = t["r32"], t["s32"]
        else:
            ok, r, s = O.der_parse_lax(t["sig"])
            if not ok:
                r = s = bytes(32)
        rows.append(dict(t, pub65=bytes([tag]) + x + y, r32=r, s32=s))
    valid = [t for t in rows if t["cls"] in ("valid_c", "valid_u", "valid_h") and t["verdict"] == 1]
    k = 0
    for cls, (rv, sv) in RAW_CLASSES.items():
        for _ in range(RAW_PER_CLASS):
            t = valid[(37 * k) % len(valid)]
            k += 1
            rows.append(dict(t, cls=cls, verdict=0, sig=b"",
                             r32=t["r32"] if rv is None else rv.to_bytes(32, "big"),
                             s32=t["s32"] if sv is None else sv.to_bytes(32, "big")))
    cols = dict(pub65=_rows2d([t["pub65"] for t in rows], 65), hash=_rows2d([t["hash"] for t in rows], 32),
                r32=_rows2d([t["r32"] for t in rows], 32), s32=_rows2d([t["s32"] for t in rows], 32),
                sig=_rows2d([t["sig"] for t in rows], max(len(t["sig"]) for t in rows)),
                siglen=np.array([len(t["sig"]) for t in rows], np.int64),
                pub=_rows2d([t["pub"] for t in rows], max(len(t["pub"]) for t in rows)),
                publen=np.array([len(t["pub"]) for t in rows], np.int64))
    _tables["ecdsa"] = Table("ecdsa", cols, [t["cls"] for t in rows], [t["verdict"] for t in rows],
                             ("valid_c", "valid_u", "valid_h"))
    return _tables["ecdsa"]


def schnorr_table():
    """structured_scalars()["schnorr"], schnorr_tuples(), the BIP340 vectors and
    schnorr_exceptional().  Columns: sig (64), msg, pub (32)."""
    if "schnorr" in _tables:
        return _tables["schnorr"]
    rows = structured_scalars()["schnorr"] + schnorr_tuples() + bip340_vectors() + schnorr_exceptional()
    cols = dict(sig=_rows2d([t["sig"] for t in rows], 64), msg=_rows2d([t["msg"] for t in rows], 32),
                pub=_rows2d([t["pub"] for t in rows], 32))
    _tables["schnorr"] = Table("schnorr", cols, [t["cls"] for t in rows], [t["verdict"] for t in rows],
                               ("valid", "valid_same_key", "valid_structured_key_nonce"))
    return _tables["schnorr"]


def table(kind):
    return ecdsa_table() if kind == "ecdsa" else schnorr_table()


# ---- chains ------------------------------------------------------------------------------------
def threads(cnt, cus, per_thread=PER_THREAD):
    """T of a batched inversion over cnt lanes, as the design states it (the module docstring)."""
    return max(-(-cnt // per_thread), min(cnt, cus * 256))


def chain_of(i, cnt, T):
    """(chain id, position, chain length) of lane i: thread t owns lanes t, t + T, ... below cnt."""
    assert 0 <= i < cnt and T >= 1
    t = i % T
    return t, i // T, (cnt - 1 - t) // T + 1


def _by_chain(values, cnt, T, fill):
    """values (one per lane) as a (positions, T) matrix: column t is chain t, padded with fill."""
    L = -(-cnt // T)
    m = np.full(L * T, fill, dtype=np.asarray(values).dtype)
    m[:cnt] = values
    return m.reshape(L, T)


def chain_coverage(tab, idx, T):
    """What the chains of one chunk hold, from the index vector alone:
    alone      {(class, position, chain length)}: a non-normal row whose chain is otherwise valid
    packed     chains (of more than one lane) whose members are all non-normal
    one_valid  {(position, chain length)}: all non-normal but one valid row, at that position
    adjacent   chains with two rows of the doubling class at consecutive positions"""
    cnt = len(idx)
    nn = _by_chain(tab.non_normal[idx], cnt, T, False)
    good = _by_chain(tab.good[idx], cnt, T, False)
    length = _by_chain(np.ones(cnt, bool), cnt, T, False).sum(0)
    nnc, gc = nn.sum(0), good.sum(0)
    alone = set()
    for t in np.flatnonzero((nnc == 1) & (gc == length - 1)):
        p = int(np.argmax(nn[:, t]))
        alone.add((tab.cls_name(idx[t + p * T]), p, int(length[t])))
    one_valid = {(int(np.argmax(good[:, t])), int(length[t]))
                 for t in np.flatnonzero((length > 1) & (nnc == length - 1) & (gc == 1))}
    dbl = _by_chain(tab.cls[idx] == tab.classes.index(DOUBLING[tab.kind]), cnt, T, False)
    return dict(alone=alone, packed=int(((length > 1) & (nnc == length)).sum()), one_valid=one_valid,
                adjacent=int((dbl[:-1] & dbl[1:]).any(0).sum()) if len(dbl) > 1 else 0)


class _Picker:
    """The rows of a class in rotation, so that repeated placements use different rows."""

    def __init__(self, tab):
        self.tab, self.at = tab, {}

    def __call__(self, cls):
        rows = self.tab.rows_of(cls)
        k = self.at.get(cls, 0)
        self.at[cls] = k + 1
        return rows[k % len(rows)]


def _scatter_table(tab, idx, free, rng):
    """Every row of the table once, at seeded random lanes among `free`."""
    lanes = rng.choice(free, size=len(tab), replace=False)
    idx[lanes] = np.arange(len(tab))
    return lanes


def expected(tab, idx):
    return tab.verdict[idx]


ALONE_AT = ((0, 16), (1, 16), (7, 16), (14, 16), (15, 16), (14, 15))  # (position, chain length)
SHORT = 37  # chains of 15 in chains_full


def chains_full(cus, kind="ecdsa", seed=0xC4A1):
    """One batch of 16 * cus * 256 - 37 rows: T = cus * 256, chains of 16, the last 37 of 15.
    Reserved chains (seeded random ids, so that they mix with other chains in their waves):
      * every non-normal class alone in an otherwise valid chain at each of ALONE_AT;
      * 64 chains of 16 and 4 of 15 all of whose members are non-normal (the product stays 1);
      * chains of 16 / of 15 with one valid row, at each position, among non-normal rows;
      * chains with two rows of the doubling class at positions (0, 1), (7, 8), (14, 15), (13, 14);
    every row of the table once more at seeded random lanes of the other chains; valid filler rows
    everywhere else."""
    tab = table(kind)
    n = PER_THREAD * cus * 256 - SHORT
    T = threads(n, cus)
    assert T == cus * 256
    rng = np.random.default_rng(seed + cus)
    idx = tab.filler[rng.integers(len(tab.filler), size=n)]
    long_ids = iter(rng.permutation(T - SHORT))
    short_ids = iter(T - SHORT + rng.permutation(SHORT))
    pick, nnc = _Picker(tab), tab.non_normal_classes
    reserved = []

    def chain(length):
        t = int(next(long_ids if length == 16 else short_ids))
        assert chain_of(t, n, T) == (t, 0, length)
        reserved.append(t)
        return t

    for c in nnc:
        for p, length in ALONE_AT:
            idx[chain(length) + p * T] = pick(c)
    k = 0
    for length, count in ((16, 64), (15, 4)):
        for _ in range(count):
            t = chain(length)
            for p in range(length):
                idx[t + p * T] = pick(nnc[k % len(nnc)])
                k += 1
    for length in (16, 15):
        for hole in range(length):
            t = chain(length)
            for p in range(length):
                if p != hole:
                    idx[t + p * T] = pick(nnc[k % len(nnc)])
                    k += 1
    for p, length in ((0, 16), (7, 16), (14, 16), (13, 15)):
        t = chain(length)
        idx[t + p * T] = pick(DOUBLING[kind])
        idx[t + (p + 1) * T] = pick(DOUBLING[kind])
    free = np.ones(n, bool)
    for t in reserved:
        free[t::T] = False
    _scatter_table(tab, idx, np.flatnonzero(free), rng)
    rec = dict(chain_coverage(tab, idx, T), n=n, T=T, kind=kind, reserved=len(reserved),
               lengths={chain_of(t, n, T)[2] for t in (0, T - SHORT - 1, T - SHORT, T - 1)},
               filler_all_valid=bool(tab.good[tab.filler].all()), rows_present=len(set(idx.tolist())))
    return idx, rec


def assert_full_coverage(rec, kind):
    """The coverage conditions of chains_full, on its record."""
    tab = table(kind)
    want = {(c, p, length) for c in tab.non_normal_classes for p, length in ALONE_AT}
    assert want <= rec["alone"], sorted(want - rec["alone"])
    assert rec["packed"] >= 64, rec["packed"]
    assert {(p, 16) for p in range(16)} | {(p, 15) for p in range(15)} <= rec["one_valid"]
    assert rec["adjacent"] >= 4, rec["adjacent"]
    assert rec["lengths"] == {15, 16} and rec["filler_all_valid"]
    assert rec["rows_present"] == len(tab)  # every fixture row is somewhere in the batch


def chunked_shape(cus):
    """(n, chunk lanes, [(base, cnt)]) of chains_chunked."""
    S = cus * 256
    C = 2 * S
    n = 2 * C + S + 19
    return n, C, [(b, min(C, n - b)) for b in range(0, n, C)]


def _chunk_slots(tab, two):
    """(class, position) pairs of a chunk with `two` chains of two lanes: every non-normal class at
    both positions where they fit, else as many as fit in NON_NORMAL's order (the exceptional sums
    first); chains left over take the doubling class again."""
    slots = [(c, p) for c in tab.non_normal_classes for p in (0, 1)][:two]
    return slots + [(DOUBLING[tab.kind], j & 1) for j in range(min(two, 24) - len(slots))]


def chains_chunked(cus, kind="ecdsa", seed=0xC4C4):
    """n = 2 * (2 * cus * 256) + cus * 256 + 19 rows for chunks of 2 * cus * 256 lanes: three
    chunks, every chain of the first two has two lanes, and the short last chunk has 19 chains of
    two.  In each chunk, chain j (lanes base + j and base + T + j, the lanes right after the
    chunk's base) holds one non-normal row and one valid row for the (class, position) pairs of
    _chunk_slots -- all of them at both positions in the first two chunks; the last chunk has room
    for 19 (BIP340: all; ECDSA: the exceptional sums at both positions, then the rejected classes
    in order).  Each chunk's last lane holds a row of the doubling class beside a valid one.  The
    whole table once more at seeded random lanes of the other chains."""
    tab = table(kind)
    n, C, chunks = chunked_shape(cus)
    rng = np.random.default_rng(seed + cus)
    idx = tab.filler[rng.integers(len(tab.filler), size=n)]
    pick = _Picker(tab)
    free = np.ones(n, bool)
    plan = []
    for base, cnt in chunks:
        T = threads(cnt, cus)
        assert T == cus * 256 and T < cnt <= 2 * T
        two = cnt - T
        slots = _chunk_slots(tab, two)
        for j, (c, p) in enumerate(slots):
            idx[base + j + p * T] = pick(c)
            free[[base + j, base + j + T]] = False
        if two > len(slots):  # the chunk's last lane: position 1 of chain two - 1
            idx[base + cnt - 1] = pick(DOUBLING[kind])
            free[[base + cnt - 1 - T, base + cnt - 1]] = False
        plan.append(slots)
    _scatter_table(tab, idx, np.flatnonzero(free), rng)
    per_chunk = []
    for (base, cnt), slots in zip(chunks, plan):
        T = threads(cnt, cus)
        cov = chain_coverage(tab, idx[base:base + cnt], T)
        first = {(tab.cls_name(idx[base + j + p * T]), p) for j, (_, p) in enumerate(slots)
                 if tab.good[idx[base + j + (1 - p) * T]]}
        per_chunk.append(dict(base=base, cnt=cnt, T=T, two=cnt - T, slots=slots, after_base=first,
                              alone={(c, p) for c, p, length in cov["alone"] if length == 2}))
    return idx, dict(n=n, chunk_lanes=C, chunks=per_chunk, kind=kind,
                     filler_all_valid=bool(tab.good[tab.filler].all()),
                     rows_present=len(set(idx.tolist())))


def assert_chunked_coverage(rec, kind):
    tab = table(kind)
    every = {(c, p) for c in tab.non_normal_classes for p in (0, 1)}
    assert [c["two"] for c in rec["chunks"]] == [rec["chunks"][0]["T"]] * 2 + [19]
    for c in rec["chunks"]:
        assert set(c["slots"]) <= c["after_base"] <= c["alone"], (c["base"], sorted(c["slots"]))
        assert len(c["slots"]) >= min(c["two"], len(every))
        if c["two"] >= len(every):
            assert every <= c["alone"], (c["base"], sorted(every - c["alone"]))
    assert rec["filler_all_valid"] and rec["rows_present"] == len(tab)


SIZE_NAMES = ("1", "2", "63", "64", "65", "wg-1", "wg", "wg+1", "cus*128-1", "cus*128", "cus*128+1",
              "cus*256-1", "cus*256", "cus*256+1", "cus*256+wg-1", "cus*256+wg+1", "2*cus*256+1",
              "R-1", "R", "R+1", "R+wg-1", "R+wg+1", "2R", "2R+1")  # sizes(), entry by entry


def sizes(cus, wg, R):
    """The row counts at which the launch shape changes: around the wave, the ladder workgroup,
    the latency-mode bound cus * 128, the first chains of two (cus * 256), and the K_keyq
    residency round R (a tail launch of one lane at R + 1, two whole rounds at 2 R)."""
    S = cus * 256
    return [1, 2, 63, 64, 65, wg - 1, wg, wg + 1, cus * 128 - 1, cus * 128, cus * 128 + 1, S - 1, S,
            S + 1, S + wg - 1, S + wg + 1, 2 * S + 1, R - 1, R, R + 1, R + wg - 1, R + wg + 1, 2 * R,
            2 * R + 1]


def size_shape(n, cus, R):
    """(mode, A) a batch of n rows is meant to take (default chunk size): latency mode up to
    cus * 128 rows; a split at the last whole residency round when n > R is no multiple of R."""
    if 2 * n <= cus * 256:
        return "latency", 0
    if n > R and n % R:
        return "split", n // R * R
    return "one_launch", 0


def size_batch(n, cus, wg, R, kind="ecdsa"):
    """n rows: the whole table recurring cyclically from a size-dependent offset; where they fit,
    the last lane, the first lane of the last workgroup and the lane at the split point A each
    hold a row of the doubling class with a rejected row beside it."""
    tab = table(kind)
    offset = (n * 2654435761) % len(tab)
    idx = (offset + np.arange(n)) % len(tab)
    pick = _Picker(tab)
    placed = []
    A = size_shape(n, cus, R)[1]
    for name, lane, step in (("last", n - 1, -1), ("last_wg", (n - 1) // wg * wg, 1), ("A", A, 1)):
        if name == "A" and A == 0:
            continue
        for k, cls in enumerate((DOUBLING[kind], REJECTED[kind])):
            at = lane + k * step
            if 0 <= at < n and at not in [p[1] for p in placed]:
                idx[at] = pick(cls)
                placed.append((name, at, cls))
    return idx, dict(n=n, offset=offset, placed=placed, A=A, kind=kind)


# ---- the commitment kernels' chain (tweak_fin_kernel) --------------------------------------------
# rows tweak_add_lane decides without comparing a point: they leave the running product alone
DECIDED = ("parity_2", "parity_255", "t_zero_par0", "t_zero_par1", "t_eq_n", "t_max", "t_n_plus_t",
           "infinity_q0", "infinity_qp", "p_off_curve", "p_eq_prime", "p_eq_prime_plus_1",
           "q_eq_prime", "q_plus_prime")


def decided_chain(mirror=False):
    """A 32-row tweak batch (T = ceil(32 / 16) = 2): every even lane holds a decided row of the
    golden commitment tuples (the reference's verdicts), every odd lane a valid row -- chain 0 never
    multiplies, chain 1 always does -- or, mirrored, the other way round.  Returns (rows, record)
    with rows = [dict(cls, q, parity, p, t, verdict)]."""
    import commit_cases as C
    tuples = C.load_golden()[1]
    by = {}
    for t in tuples:
        by.setdefault(t["cls"][4:] if t["cls"].startswith("mix_") else t["cls"], []).append(t)
    dec = [by[c][0] for c in DECIDED if c in by]
    assert len(dec) >= 12, sorted(by)
    dec = (dec + [by[c][-1] for c in DECIDED if c in by])[:16]
    valid = [t for t in by["valid"] if t["verdict"] == 1][:16]
    assert len(dec) == 16 and len(valid) == 16
    rows = []
    for d, v in zip(dec, valid):
        rows += [v, d] if mirror else [d, v]
    T = 2
    rec = dict(n=len(rows), T=T, decided_lanes=[i for i, t in enumerate(rows) if t in dec],
               classes={t["cls"] for t in dec},
               chains={chain_of(i, len(rows), T)[0] for i, t in enumerate(rows) if t in dec})
    return rows, rec


def mismatches(tab, idx, got, T, base=0, limit=20):
    """[(class, lane, chain id, position, chain length, got, expected)] of the first mismatches of
    a chunk's verdicts."""
    got = np.frombuffer(bytes(got), np.uint8)
    exp = expected(tab, idx)
    return [(tab.cls_name(idx[i]), base + int(i), *chain_of(int(i), len(idx), T), int(got[i]), int(exp[i]))
            for i in np.flatnonzero(got != exp)[:limit]]
