"""What the Taproot host-path tests share (test_taproot_hostpath.py on the device-less engine,
test_taproot_hostpath_gpu.py on librbc_amd.so): the library setters bound for either build, the
golden inputs, and the injected-fault sequence with the counters each step must leave."""
import contextlib
import ctypes

import bitcoinconsensus_amd as B
import mixed_input_cases as M
import taproot_spend_cases as S

HOST_ALL = 1 << 30          # a small-round threshold no test batch reaches
LAUNCH_FAILURE = 719        # hipErrorLaunchFailure: never retried
F = M.ALL | M.TAPROOT


def bind(L):
    """The setters and counters these tests call, with their C types, on either build."""
    L = B.lib() if L is None else L
    B._bind_consensus(L)
    B._bind_inputs(L)
    L.bcc_set_spend_round.argtypes = [ctypes.c_size_t]
    return L


@contextlib.contextmanager
def settings(L, small_round=0, spend_round=0):
    """The small-round threshold and the spend round size for one block; the suite's settings
    (threshold 0, default rounds, no injection, the default policy) are restored afterwards."""
    L = bind(L)
    try:
        L.bcc_set_host_small_round(small_round)
        L.bcc_set_spend_round(spend_round)
        yield L
    finally:
        L.bcc_debug_fail_device_rounds(0)
        L.bcc_set_device_failure_policy(B.DEVICE_FAILURE_HOST)
        L.bcc_set_spend_round(0)
        L.bcc_set_host_small_round(0)


def spend_golden():
    cases = S.load_golden()
    return S.items_of(cases), [tuple(c["expected"]) for c in cases]


def mixed_golden():
    cases = M.mixed_cases()
    return cases, M.items_of(cases), [tuple(c["expected"]) for c in cases]


def batch_stats(L):
    s = B.BatchStats()
    L.bcc_last_batch_stats(ctypes.byref(s))
    return s


def run_spends(L, items):
    """bcc_taproot_spend_batch as is: (rc, [(ret, serror)])."""
    n = len(items)
    arr, keep = B.input_items(items)
    ret, err = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    L.bcc_taproot_spend_batch.argtypes = [ctypes.POINTER(B.TaprootSpend), ctypes.c_size_t,
                                          ctypes.POINTER(ctypes.c_int),
                                          ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    rc = L.bcc_taproot_spend_batch(arr, n, ret, err, 0)
    return rc, [(ret[i], err[i]) for i in range(n)]


def fault_sequence(library=None):
    """The injected-fault steps of the issue on the spend goldens, on the v1 inputs of the mixed
    goldens (one side: every count is exact) and on the whole mixed goldens (both sides take from
    the one injection counter at the same time, so the counts are exact only in their sum), with
    the threshold at 0 and 64-item spend rounds.  Asserts results and counters; the caller restores
    nothing: settings() does."""
    with settings(library, small_round=0, spend_round=64) as L:
        spends, spends_want = spend_golden()
        cases, mixed, mixed_want = mixed_golden()
        v1 = [it for it, c in zip(mixed, cases) if c["v1"]]
        v1_want = [w for w, c in zip(mixed_want, cases) if c["v1"]]
        assert len(spends) > 3 * 64 and len(v1) > 64 and len(mixed) > len(v1) + 64

        def run_spend():
            rc, out = run_spends(L, spends)
            return rc, out, spends_want

        def run_v1():
            rc, out = B.verify_inputs_batch_raw(v1, F, library=L)
            return (0 if rc >= 0 else rc), out, v1_want

        def run_mixed():
            rc, out = B.verify_inputs_batch_raw(mixed, F, library=L)
            return (0 if rc >= 0 else rc), out, mixed_want

        def counters(both_sides):
            t = B.last_taproot_stats(library=L)
            retries, host_rounds = t["device_retries"], t["host_rounds"]
            if both_sides:
                b = batch_stats(L)
                retries, host_rounds = retries + b.device_retries, host_rounds + b.host_rounds
            return retries, host_rounds, t

        for run, both in ((run_spend, False), (run_v1, False), (run_mixed, True)):
            def step(inject, allowed):
                """One call under `inject`: exact results, (retries, host rounds) one of `allowed`,
                and the process-wide fallback counter up by the host rounds."""
                before = L.bcc_host_fallback_rounds()
                inject()
                try:
                    rc, out, want = run()
                finally:
                    L.bcc_debug_fail_device_rounds(0)
                assert rc == 0 and out == want, (run.__name__, rc)
                retries, host_rounds, t = counters(both)
                assert (retries, host_rounds) in allowed, (run.__name__, retries, host_rounds, t)
                assert L.bcc_host_fallback_rounds() - before == host_rounds
                return t

            t = step(lambda: None, [(0, 0)])
            assert t["rounds"] >= 2 and t["host_checks"] == 0
            assert t["checks"] > 0 and t["commits"] > 0
            rounds = t["rounds"]
            step(lambda: L.bcc_debug_fail_device_rounds(1), [(1, 0)])
            # two faults: the round and its re-run; with two sides drawing from the one counter
            # they may also be one fault each, and then both re-runs succeed
            step(lambda: L.bcc_debug_fail_device_rounds(2), [(1, 1), (2, 0)] if both else [(1, 1)])
            step(lambda: L.bcc_debug_fail_device_rounds_code(1, LAUNCH_FAILURE), [(0, 1)])
            before = L.bcc_host_fallback_rounds()
            L.bcc_debug_fail_device_rounds_code(1 << 20, LAUNCH_FAILURE)
            try:
                rc, out, want = run()
            finally:
                L.bcc_debug_fail_device_rounds(0)
            assert rc == 0 and out == want, run.__name__
            t = B.last_taproot_stats(library=L)
            assert t["host_rounds"] == t["rounds"] == rounds and t["device_retries"] == 0
            assert t["host_checks"] == t["checks"] + t["commits"]
            assert L.bcc_host_fallback_rounds() - before >= rounds

            # BCC_DEVICE_FAILURE_ERROR: three faults fail one round and its re-run
            L.bcc_set_device_failure_policy(B.DEVICE_FAILURE_ERROR)
            before = L.bcc_host_fallback_rounds()
            L.bcc_debug_fail_device_rounds(3)
            try:
                rc, out, want = run()
            finally:
                L.bcc_debug_fail_device_rounds(0)
                L.bcc_set_device_failure_policy(B.DEVICE_FAILURE_HOST)
            assert rc == -1, run.__name__
            assert L.bcc_host_fallback_rounds() == before
            if run is not run_spend:  # the inputs contract: no verdict is err 6, the rest is whole
                lost = {i for i, o in enumerate(out) if o == (0, B.ERR_DEVICE_FAILURE)}
                assert lost and all(o == w for i, (o, w) in enumerate(zip(out, want))
                                    if i not in lost), run.__name__
            if run is run_mixed:
                # three faults fail exactly one side (the other's re-run finds the counter empty):
                # the lost items are all v1 with every non-v1 item intact, or all non-v1 with
                # every v1 item intact
                v1_idx = {i for i, c in enumerate(cases) if c["v1"]}
                assert lost <= v1_idx or not (lost & v1_idx), sorted(lost)[:10]
            rc, out, want = run()  # the next call, with no injection, is whole again
            assert rc == 0 and out == want, run.__name__
            assert counters(both)[:2] == (0, 0)
    return True
