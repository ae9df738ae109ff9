"""What the header tests share (test_headers_host.py on the device-less engine, where a device round
is the host evaluation behind the device seam; test_headers_gpu.py on librbc_amd.so): the cases,
built once from seeded mined chains, each run through one build of the C ABI on the device route
(small-round threshold 0) and on the host route (a threshold above every batch) and compared
exactly with tests/header_model.py."""
import contextlib
import ctypes
import functools
import random

import bitcoinconsensus_amd as B
import header_model as M

SEED = 20240611
HOST_ALL = 1 << 30          # a small-round threshold no test batch reaches
LAUNCH_FAILURE = 719        # hipErrorLaunchFailure: never retried
SPACING = 1             # seconds: 4 * timespan * the easiest target stays below 2^256
LOW_BITS = 0x2000ffff       # about 256 tries per header
LOW_LIMIT = M.set_compact(LOW_BITS)[0]
# interval 16; the gates far above every test height unless a case sets them
PARAMS = dict(pow_limit=LOW_LIMIT, timespan=16 * SPACING, spacing=SPACING, no_retargeting=False,
              bip34=1 << 30, bip66=1 << 30, bip65=1 << 30)
T0 = 1_600_000_000


def bind(L):
    L = B.lib() if L is None else L
    B._bind_consensus(L)
    B._bind_headers(L)
    return L


@contextlib.contextmanager
def settings(L, small_round=0, header_round=0):
    """The thresholds for one block of code; the suite's settings (threshold 0, default rounds, no
    injection, the default policy) are restored afterwards."""
    L = bind(L)
    try:
        L.bcc_set_host_small_round(small_round)
        L.bcc_set_header_round(header_round)
        yield L
    finally:
        L.bcc_debug_fail_device_rounds(0)
        L.bcc_set_device_failure_policy(B.DEVICE_FAILURE_HOST)
        L.bcc_set_header_round(0)
        L.bcc_set_host_small_round(0)


ROUTES = (("device", dict(small_round=0)), ("host", dict(small_round=HOST_ALL)))


def c_params(p):
    return B.HeaderParams.make(p["pow_limit"], p["timespan"], p["spacing"], p.get("no_retargeting", False),
                               False, p.get("bip34", 0), p.get("bip66", 0), p.get("bip65", 0))


def c_anchor(a):
    return None if a is None else B.HeaderAnchor.make(a["height"], a["hash"], a["bits"], a["times"],
                                                      a["period_first_time"])


def run(L, headers, params, anchor=None, max_time=0, device=0):
    return B.check_headers(headers, c_params(params), c_anchor(anchor), max_time, device, library=L)


def expect_route(st, route, n, rounds=None):
    assert st["headers"] == n and st["device_retries"] == 0, st
    if route == "device":
        assert st["host_rounds"] == 0 and st["device_rounds"] >= 1, st
    else:
        assert st["device_rounds"] == 0 and st["host_rounds"] >= 1, st
    if rounds is not None:
        assert st["device_rounds"] + st["host_rounds"] == rounds, st


def check_case(L, case, rounds=(0,)):
    """One case on both routes and every round size against the model; returns the model's result."""
    label, headers, params, anchor, max_time = case
    want = M.check(headers, params, anchor, max_time)
    for route, kw in ROUTES:
        for per in rounds:
            with settings(L, header_round=per, **kw):
                got = run(L, headers, params, anchor, max_time)
                st = B.last_header_stats(library=L)
            for k in ("first_invalid", "status", "chain_work", "hashes"):
                assert got[k] == want[k], (label, route, per, k, got["status"], want["status"])
            expect_route(st, route, len(headers), -(-len(headers) // per) if per else 1)
    return want


# ---- building chains ------------------------------------------------------------------------------


class Builder:
    """Appends mined headers that follow the model's rules unless a field is overridden."""

    def __init__(self, params, anchor=None, seed=0):
        self.p, self.anchor, self.headers = params, anchor, []
        self.rng = random.Random(SEED + seed)

    def parsed(self, k):
        return M.fields(self.headers[k])

    def height(self):
        return (self.anchor["height"] + 1 if self.anchor else 0) + len(self.headers)

    def times_before(self):
        back = [self.parsed(k)[3] for k in range(len(self.headers) - 1, -1, -1)]
        return back + (list(self.anchor["times"]) if self.anchor else [])

    def median(self):
        w = sorted(self.times_before()[:11])
        return w[len(w) // 2]

    def prev_hash(self):
        if self.headers:
            return M.sha256d(self.headers[-1])
        return self.anchor["hash"] if self.anchor else bytes(32)

    def want_bits(self):
        i, interval = len(self.headers), self.p["timespan"] // self.p["spacing"]
        if not self.headers and not self.anchor:
            return LOW_BITS
        prev_bits = self.parsed(i - 1)[4] if i else self.anchor["bits"]
        if self.height() % interval:
            return prev_bits
        first = self.parsed(i - interval)[3] if i >= interval else self.anchor["period_first_time"]
        return M.next_work(prev_bits, self.times_before()[0], first, self.p["timespan"],
                           self.p["pow_limit"], self.p.get("no_retargeting", False))

    def add(self, time=None, version=4, bits=None, prev=None, mined=True):
        before = self.times_before()
        time = (before[0] + SPACING if before else T0) if time is None else time
        bits = self.want_bits() if bits is None else bits
        prev = self.prev_hash() if prev is None else prev
        make = M.mine if mined else M.unmine
        self.headers.append(make(version, prev, self.rng.randbytes(32), time, bits, self.p["pow_limit"]))
        return self


def anchor_at(height, bits=LOW_BITS, times=None, first=T0, seed=0):
    """An anchor whose ancestors came SPACING apart, unless times (newest first) says otherwise."""
    n = min(11, height + 1)
    times = [T0 + SPACING * (height - k) for k in range(n)] if times is None else list(times)
    return dict(height=height, hash=random.Random(SEED + 100 + seed).randbytes(32), bits=bits,
                times=times, period_first_time=first)


@functools.lru_cache(maxsize=None)
def base_chain():
    """257 headers from a genesis, SPACING apart: every 16th retargets by 15/16, so the bits change
    at every boundary (index 64 among them, its period's first block inside the batch)."""
    b = Builder(PARAMS, seed=1)
    for _ in range(257):
        b.add()
    assert len({M.fields(h)[4] for h in b.headers}) == 17
    return tuple(b.headers)


@functools.lru_cache(maxsize=None)
def long_chain():
    """600 headers without retargeting: enough for two device shares."""
    p = dict(PARAMS, no_retargeting=True)
    b = Builder(p, seed=2)
    for _ in range(600):
        b.add()
    return tuple(b.headers), p


def remined(headers, k, **change):
    """headers with header k's fields changed and mined again (the header after it keeps naming the
    old hash)."""
    version, prev, merkle, time, bits, _ = M.fields(headers[k])
    f = dict(version=version, prev=prev, merkle=merkle, time=time, bits=bits)
    mined = change.pop("mined", True)
    f.update(change)
    h = (M.mine if mined else M.unmine)(f["version"], f["prev"], f["merkle"], f["time"], f["bits"], LOW_LIMIT)
    return list(headers[:k]) + [h] + list(headers[k + 1:])


# ---- the cases --------------------------------------------------------------------------------------


def check_lane_geometry(L):
    base = list(base_chain())
    for n in (1, 63, 64, 65, 257):
        want = check_case(L, (f"n={n}", base[:n], PARAMS, None, 0))
        assert want["first_invalid"] == n and want["chain_work"] > 0
    # a median-time window and a retarget across two cuts; a boundary as a round's first header
    want = check_case(L, ("40 in rounds of 7", base[:40], PARAMS, None, 0), rounds=(7, 16))
    assert want["status"] == [M.OK] * 40
    check_case(L, ("65 in rounds of 64", base[:65], PARAMS, None, 0), rounds=(64,))
    # the same chain continued from an anchor inside it: every context field comes from the anchor
    for cut in (1, 5, 16, 17, 40):
        times = [M.fields(base[k])[3] for k in range(cut - 1, max(cut - 12, -1), -1)]
        first = M.fields(base[(cut + 15) // 16 * 16 - 16])[3]
        a = dict(height=cut - 1, hash=M.sha256d(base[cut - 1]), bits=M.fields(base[cut - 1])[4],
                 times=times, period_first_time=first)
        want = check_case(L, (f"anchor at {cut - 1}", base[cut:cut + 60], PARAMS, a, 0), rounds=(0, 7))
        assert want["status"] == [M.OK] * 60, (cut, want["status"])


def check_device_list(L, set_devices):
    headers, p = long_chain()
    want = M.check(headers, p)
    assert want["first_invalid"] == 600
    with settings(L):
        one = run(L, headers, p, device=0)
        set_devices([0, 0])
        try:
            two = run(L, headers, p, device=-1)
            st = B.last_header_stats(library=L)
        finally:
            set_devices([0])
    assert one == two == want
    assert st["device_rounds"] == 2 and st["headers"] == 600, st


def pow_rows():
    """(hash, bits) rows: every exponent 0..36 with the mantissas below; for each target that is
    valid under the widest limit the hash equal to it, one above and below, and one limb alone one
    above and below."""
    rows = []
    for size in range(37):
        for mant in (0, 1, 0xff, 0x100, 0xffff, 0x10000, 0x7fffff, 0x800000, 0x800001):
            bits = size << 24 | mant
            target, negative, overflow = M.set_compact(bits)
            hashes = {0, target & M.MASK}
            if not (negative or overflow or target == 0):
                hashes |= {target - 1, min(target + 1, M.MASK)}
                for limb in range(8):
                    w = target >> 32 * limb & 0xffffffff
                    if w < 0xffffffff:
                        hashes.add(target + (1 << 32 * limb))
                    if w > 0:
                        hashes.add(target - (1 << 32 * limb))
            rows += [(h.to_bytes(32, "little"), bits) for h in sorted(hashes)]
    return rows


def check_compact_targets(L):
    L = bind(L)
    rows = pow_rows()
    assert len(rows) > 2000
    mainnet = 0xffff << 208     # its top limb is zero
    limits = [M.MASK, (1 << 255) - 1, LOW_LIMIT, LOW_LIMIT - 1, mainnet, mainnet - 1, 0]
    extra = []
    for lim in (LOW_LIMIT, mainnet):  # the target equal to the limit, at limit and limit - 1 above
        bits = M.get_compact(lim)
        assert M.set_compact(bits)[0] == lim
        extra += [(lim.to_bytes(32, "little"), bits), ((lim + 1).to_bytes(32, "little"), bits),
                  (bytes(32), bits)]
    rows = rows + extra
    blob = b"".join(h for h, _ in rows)
    bits = [b for _, b in rows]
    for limit in limits:
        want = bytes(M.check_pow(h, b, limit) for h, b in rows)
        assert limit == 0 or 0 < sum(want) < len(rows)
        for route, kw in ROUTES:
            for per in (0, 1000):
                with settings(L, header_round=per, **kw):
                    got = B.pow_check_tuples(blob, bits, limit, library=L)
                    st = B.last_header_stats(library=L)
                bad = [(i, hex(bits[i])) for i in range(len(rows)) if got[i] != want[i]]
                assert not bad, (route, hex(limit), bad[:10])
                expect_route(st, route, len(rows), -(-len(rows) // per) if per else 1)
    assert B.pow_check_tuples(b"", [], LOW_LIMIT, library=L) == b""
    f = L.mi_pow_check_tuples
    one, lim, out = (ctypes.c_uint32 * 1)(LOW_BITS), bytes(32), ctypes.create_string_buffer(1)
    assert f(None, one, 1, lim, out, 0) == -1 and f(bytes(32), None, 1, lim, out, 0) == -1
    assert f(bytes(32), one, 1, None, out, 0) == -1 and f(bytes(32), one, 1, lim, None, 0) == -1
    assert f(None, None, 0, None, None, 0) == 0


def retarget_cases():
    """A boundary at index 0 on an anchor at height 15, its period's first block before the batch:
    one header per case with the bits the rule demands, and one that keeps the old bits."""
    span = PARAMS["timespan"]
    last = T0 + 20 * span
    cases = []

    def one(label, actual, bits=LOW_BITS, params=PARAMS, expect=None):
        a = anchor_at(15, bits=bits, times=[last - 7 * k for k in range(11)], first=last - actual)
        b = Builder(params, a, seed=len(cases))
        want = b.want_bits()
        assert expect is None or expect(want), (label, hex(want))
        cases.append((label, b.add(time=last + 1).headers, params, a, 0))
        if want != bits:
            cases.append((label + ", old bits kept", Builder(params, a, seed=len(cases)).add(
                time=last + 1, bits=bits).headers, params, a, 0))

    q = M.set_compact(0x1f00ffff)[0]
    one("span/4", span // 4, bits=0x1f3fffc0, expect=lambda w: w == M.get_compact(M.set_compact(0x1f3fffc0)[0] // 4))
    one("span/4 - 1 clamps", span // 4 - 1, bits=0x1f3fffc0,
        expect=lambda w: w == M.get_compact(M.set_compact(0x1f3fffc0)[0] // 4))
    one("span/4 + 1", span // 4 + 1, bits=0x1f3fffc0,
        expect=lambda w: w != M.get_compact(M.set_compact(0x1f3fffc0)[0] // 4))
    one("4 span", 4 * span, bits=0x1f00ffff, expect=lambda w: w == M.get_compact(4 * q))
    one("4 span + 1 clamps", 4 * span + 1, bits=0x1f00ffff, expect=lambda w: w == M.get_compact(4 * q))
    one("4 span - 1", 4 * span - 1, bits=0x1f00ffff, expect=lambda w: w != M.get_compact(4 * q))
    one("last before first", -5000, bits=0x1f3fffc0,
        expect=lambda w: w == M.get_compact(M.set_compact(0x1f3fffc0)[0] // 4))
    one("result above the limit", 4 * span, expect=lambda w: w == LOW_BITS)
    # 0xffff * 0.6 = 0x9999: the mantissa's top bit is set and GetCompact moves it down a byte
    one("renormalised", span * 6 // 10, expect=lambda w: w >> 24 == 0x20 and w & 0x00ff0000 == 0 and
        w & 0xffff >= 0x8000)
    wide = dict(PARAMS, pow_limit=(1 << 255) - 1)
    one("product past 256 bits", 4 * span, bits=0x207fffff, params=wide,
        expect=lambda w: M.set_compact(w)[0] < M.set_compact(0x207fffff)[0])
    one("no retargeting", span // 4, params=dict(PARAMS, no_retargeting=True), expect=lambda w: w == LOW_BITS)
    return cases


def check_retargets(L):
    for case in retarget_cases():
        want = check_case(L, case)
        assert want["status"] == [M.BAD_DIFFBITS if "old bits" in case[0] else M.OK], (case[0], want)
    # the anchor itself is the period's first block (height 0), the boundary is header 15
    a = anchor_at(0, times=[T0], first=T0)
    b = Builder(PARAMS, a, seed=40)
    for _ in range(20):
        b.add()
    want = check_case(L, ("anchor is the period's first", b.headers, PARAMS, a, 0), rounds=(0, 7))
    assert want["status"] == [M.OK] * 20 and M.fields(b.headers[15])[4] != LOW_BITS


def check_times(L):
    rng = random.Random(SEED + 3)
    hi = 1 << 31
    for height in range(12):      # the header has height + 1 and min(11, height + 1) times before it
        times = [rng.choice((hi - 2, hi - 1, hi, hi + 1, hi + 5, hi + 5)) for _ in range(height + 1)][:11]
        a = anchor_at(height, times=times, seed=height)
        median = sorted(times)[len(times) // 2]
        for t, status in ((median, M.TIME_TOO_OLD), (median + 1, M.OK), (0xffffffff, M.OK)):
            h = Builder(PARAMS, a, seed=50 + height).add(time=t).headers
            want = check_case(L, (f"height {height + 1} time {t - median:+d}", h, PARAMS, a, 0))
            assert want["status"] == [status], (height, times, t, want)
    # inside a batch: unsorted and equal times, 0 to 11 predecessors, at and above 2^31
    b = Builder(PARAMS, seed=4)
    b.add(time=hi - 3)
    for k in range(30):
        b.add(time=b.median() + 1 + (k * 7) % 3)
    ts = [M.fields(h)[3] for h in b.headers]
    assert ts != sorted(ts) and len(set(ts)) < len(ts) and max(ts) > hi
    want = check_case(L, ("jittering times", b.headers, PARAMS, None, 0), rounds=(0, 7))
    assert want["status"] == [M.OK] * 31
    for k in (1, 5, 12, 21):
        bb = Builder(PARAMS, seed=4)
        bb.headers = list(b.headers[:k])
        bb.add(time=bb.median())
        hs = bb.headers + list(b.headers[k + 1:])
        want = check_case(L, (f"time == median at {k}", hs, PARAMS, None, 0), rounds=(0, 7))
        assert want["status"][k] == M.TIME_TOO_OLD and want["first_invalid"] == k
        assert want["status"][k + 1] == M.PREV_MISMATCH
    # the caller's bound
    j = 20
    for max_time, status in ((ts[j], M.OK), (ts[j] - 1, M.TIME_TOO_NEW), (0, M.OK)):
        want = check_case(L, (f"max_time {max_time}", b.headers[:j + 1], PARAMS, None, max_time))
        assert want["status"][j] == status, (max_time, want["status"])


def check_versions(L):
    p = dict(PARAMS, bip34=5, bip66=8, bip65=11)
    a = anchor_at(2)
    for version in (-1, 1, 2, 3, 4):
        b = Builder(p, a, seed=60 + version)
        for _ in range(10):       # heights 3..12: both sides of each gate
            b.add(version=version)
        want = check_case(L, (f"version {version}", b.headers, p, a, 0), rounds=(0, 3))
        gate = {-1: 5, 1: 5, 2: 8, 3: 11, 4: 99}[version]
        assert want["status"] == [M.OK if 3 + k < gate else M.BAD_VERSION for k in range(10)], want


def check_linkage(L):
    base = list(base_chain())
    wrong = bytes(31) + b"\x01"
    a = anchor_at(7)
    h = Builder(PARAMS, a, seed=70).add(prev=wrong).headers
    assert check_case(L, ("wrong prev at 0 on an anchor", h, PARAMS, a, 0))["status"] == [M.PREV_MISMATCH]
    for k, n, rounds in ((64, 80, (0,)), (7, 40, (7,)), (14, 40, (7,))):
        hs = remined(base[:n], k, prev=wrong)
        want = check_case(L, (f"wrong prev at {k}", hs, PARAMS, None, 0), rounds=rounds)
        assert want["status"][k] == want["status"][k + 1] == M.PREV_MISMATCH and want["first_invalid"] == k
        assert want["status"][k + 2] == M.OK
        assert want["chain_work"] == sum(M.block_proof(M.fields(x)[4]) for x in hs[:k])


def check_order_and_work(L):
    base = list(base_chain())
    wrong = bytes(31) + b"\x02"
    k = 20
    version, prev, merkle, time, bits, _ = M.fields(base[k])
    old = M.fields(base[k - 8])[3]
    p = dict(PARAMS, bip34=0, bip66=0, bip65=0)
    for label, change, max_time, status in (
            ("high hash, wrong prev", dict(prev=wrong, mined=False), 0, M.HIGH_HASH),
            ("wrong prev, wrong bits", dict(prev=wrong, bits=0x2000fffe), 0, M.PREV_MISMATCH),
            ("wrong bits, too old", dict(bits=0x2000fffe, time=old), 0, M.BAD_DIFFBITS),
            ("too old, too new, bad version", dict(time=old, version=1), 1, M.TIME_TOO_OLD),
            ("too new, bad version", dict(version=1), time - 1, M.TIME_TOO_NEW),
            ("bad version", dict(version=1), time, M.BAD_VERSION)):
        hs = remined(base[:k + 2], k, **change)
        want = check_case(L, (label, hs, p, None, max_time))
        assert want["status"][k] == status, (label, want["status"])
        assert max_time in (0, time) or want["first_invalid"] <= k
    # first invalid at 0, in the middle, absent; the work of a chain whose bits change
    hs = remined(base[:3], 0, mined=False)
    want = check_case(L, ("a genesis without proof of work", hs, PARAMS, None, 0))
    assert want["first_invalid"] == 0 and want["chain_work"] == 0 and want["status"][0] == M.HIGH_HASH
    want = check_case(L, ("every header passes", base[:100], PARAMS, None, 0), rounds=(0, 33))
    proofs = [M.block_proof(M.fields(x)[4]) for x in base[:100]]
    assert want["first_invalid"] == 100 and want["chain_work"] == sum(proofs) and len(set(proofs)) == 7
    hs = remined(base[:100], 50, version=1)
    want = check_case(L, ("a prefix up to a bad version", hs, p, None, 0))
    assert want["first_invalid"] == 50 and want["chain_work"] == sum(proofs[:50])


ALL_CHECKS = (check_lane_geometry, check_compact_targets, check_retargets, check_times, check_versions,
              check_linkage, check_order_and_work)


def fault_sequence(library=None):
    """bcc_debug_fail_device_rounds against the header rounds: one fault is retried, two fall back
    to the host, a sticky code goes straight to the host, and BCC_DEVICE_FAILURE_ERROR returns an
    error; every delivered result is the model's."""
    base = list(base_chain())[:100]
    want = M.check(base, PARAMS)
    rows = pow_rows()[:500]
    blob, bits = b"".join(h for h, _ in rows), [b for _, b in rows]
    pow_want = bytes(M.check_pow(h, b, LOW_LIMIT) for h, b in rows)
    with settings(library) as L:
        def run_headers():
            assert run(L, base, PARAMS) == want

        def run_pow():
            assert B.pow_check_tuples(blob, bits, LOW_LIMIT, library=L) == pow_want

        for f in (run_headers, run_pow):
            for inject, retries, host_rounds in (
                    (lambda: None, 0, 0),
                    (lambda: L.bcc_debug_fail_device_rounds(1), 1, 0),
                    (lambda: L.bcc_debug_fail_device_rounds(2), 1, 1),
                    (lambda: L.bcc_debug_fail_device_rounds_code(1, LAUNCH_FAILURE), 0, 1),
                    (lambda: L.bcc_debug_fail_device_rounds_code(1 << 20, LAUNCH_FAILURE), 0, 1)):
                before = L.bcc_host_fallback_rounds()
                inject()
                try:
                    f()
                finally:
                    L.bcc_debug_fail_device_rounds(0)
                st = B.last_header_stats(library=L)
                assert (st["device_retries"], st["host_rounds"]) == (retries, host_rounds), (f.__name__, st)
                assert st["device_rounds"] == 1 - host_rounds, (f.__name__, st)
                assert L.bcc_host_fallback_rounds() - before == host_rounds
            L.bcc_set_device_failure_policy(B.DEVICE_FAILURE_ERROR)
            before = L.bcc_host_fallback_rounds()
            L.bcc_debug_fail_device_rounds(3)
            try:
                try:
                    f()
                    raise AssertionError("no error under BCC_DEVICE_FAILURE_ERROR")
                except RuntimeError:
                    pass
            finally:
                L.bcc_debug_fail_device_rounds(0)
                L.bcc_set_device_failure_policy(B.DEVICE_FAILURE_HOST)
            assert L.bcc_host_fallback_rounds() == before
            f()  # the next call, with no injection, is whole again
            st = B.last_header_stats(library=L)
            assert (st["device_retries"], st["host_rounds"]) == (0, 0), st
    return True
