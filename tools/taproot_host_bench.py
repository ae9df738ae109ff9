#!/usr/bin/env python3
"""Measure the Taproot side's host path against its device path and write one JSON file under
profiles/taproot_host/.

    python3 tools/taproot_host_bench.py [--calls 200] [--reps 30] [--out profiles/taproot_host/...]

Three measurements, all in one process after a warm-up of both paths:
  lone_input   one bcc_verify_input on a key-path v1 input with the small-round threshold at its
               default (the host verifies it) and at 0 (a device round), the two interleaved call
               by call: median and spread of `--calls` calls each.
  host_rate    4,096 key-path checks through bcc_taproot_verify_batch with every round on the host,
               at 1 host thread and at bcc_get_host_threads(): checks per second.
  crossover    the same checks in batches of 1, 2, 4, ..., 256 on both paths (`--reps` calls each,
               interleaved): the smallest size at which the device's median is below the host's.
The checks are the key-path signature checks of tests/golden/taproot_checks.json.gz that reach
BIP340 (valid and invalid), tiled.  The tool has no pass mark; it asserts only that both paths
give the same answers.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rust-bitcoinconsensus_amd"), os.path.join(ROOT, "tests")]
import bitcoinconsensus_amd as B  # noqa: E402
import taproot_spend_cases as S  # noqa: E402
from fixtures import taproot_checks  # noqa: E402

HOST_ALL = 1 << 30


def spread(ts):
    ts = sorted(ts)
    q = lambda p: ts[min(len(ts) - 1, int(p * len(ts)))]  # noqa: E731
    return dict(calls=len(ts), median_ms=1e3 * statistics.median(ts), min_ms=1e3 * ts[0],
                p10_ms=1e3 * q(0.10), p90_ms=1e3 * q(0.90), max_ms=1e3 * ts[-1])


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--checks", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "taproot_host",
                                                  "taproot_host_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("taproot_host_bench.py needs a GPU: it compares the host path with it")

    pool = [c for c in taproot_checks() if c["sigversion"] == B.SIGVERSION_TAPROOT
            and c["ret"] != -1 and c["serror"] in (0, B.SCRIPT_ERR_SCHNORR_SIG)]
    checks = (pool * (a.checks // len(pool) + 1))[:a.checks]
    want = [(c["ret"], c["serror"]) for c in checks]
    gold = S.load_golden()
    lone = next(c for c in gold if c["cls"].startswith("s_keypath") and tuple(c["expected"]) == (1, 0))

    def verify_input():
        return B.verify_input(lone["tx"], lone["spent"], lone["nin"])

    def batch(n):
        return B.taproot_verify_batch(checks[:n])

    def on(path):
        B.set_host_small_round(HOST_ALL if path == "host" else 0)

    doc = dict(tool="tools/taproot_host_bench.py", source_hash=B.source_hash(),
               device=torch.cuda.get_device_name(0), host_threads=B.host_threads(),
               cpu_share=B.cpu_share(), key_path_checks_in_pool=len(pool),
               small_round_default=B.HOST_SMALL_ROUND_DEFAULT)
    # warm-up: comb tables, contexts, code objects, both paths
    for path in ("host", "device"):
        on(path)
        assert batch(256) == want[:256]
        assert verify_input() == (1, 0)

    # 1. a lone input, the two thresholds interleaved
    times = {"default": [], "zero": []}
    where = {}
    for _ in range(a.calls):
        for name, thr in (("default", B.HOST_SMALL_ROUND_DEFAULT), ("zero", 0)):
            B.set_host_small_round(thr)
            dt, r = timed(verify_input)
            assert r == (1, 0)
            times[name].append(dt)
            where[name] = B.last_taproot_stats()["host_rounds"]
    assert where == {"default": 1, "zero": 0}, where
    doc["lone_input"] = dict(input=lone["cls"],
                             threshold_default_host=spread(times["default"]),
                             threshold_0_device=spread(times["zero"]))

    # 2. the host path's rate
    on("host")
    rate = {}
    for name, threads in (("1_thread", 1), (f"{B.host_threads()}_threads", 0)):
        B.set_host_threads(threads)
        batch(len(checks))
        ts = []
        for _ in range(5):
            dt, r = timed(lambda: batch(len(checks)))
            assert r == want
            ts.append(dt)
        st = B.last_taproot_stats()
        assert st["host_rounds"] == st["rounds"] and st["host_checks"] == len(checks)
        rate[name] = dict(checks=len(checks), checks_per_s=len(checks) / statistics.median(ts),
                          **spread(ts))
    B.set_host_threads(0)
    doc["host_rate"] = dict(rate, note="whole bcc_taproot_verify_batch calls from Python: the "
                                       "item array is built per call, the job build and SHA-256 "
                                       "are inside")
    # (the device on the same batch, for scale)
    on("device")
    batch(len(checks))
    ts = [timed(lambda: batch(len(checks)))[0] for _ in range(5)]
    doc["device_rate"] = dict(checks=len(checks), checks_per_s=len(checks) / statistics.median(ts),
                              **spread(ts))

    # 3. where the device overtakes the host
    sizes = [1 << k for k in range(9)]
    cross = []
    for n in sizes:
        t = {"host": [], "device": []}
        for _ in range(a.reps):
            for path in ("host", "device"):
                on(path)
                dt, r = timed(lambda: batch(n))
                assert r == want[:n]
                t[path].append(dt)
        cross.append(dict(size=n, host=spread(t["host"]), device=spread(t["device"])))
    faster = [c["size"] for c in cross if c["device"]["median_ms"] < c["host"]["median_ms"]]
    doc["crossover"] = dict(sizes=cross, device_faster_from=faster[0] if faster else None,
                            note="medians of whole calls; device_faster_from: the smallest "
                                 "measured size whose device median is below the host's")
    B.set_host_small_round(0)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(dict(lone_host_ms=doc["lone_input"]["threshold_default_host"]["median_ms"],
                          lone_device_ms=doc["lone_input"]["threshold_0_device"]["median_ms"],
                          host_checks_per_s={k: v["checks_per_s"] for k, v in rate.items()},
                          device_checks_per_s=doc["device_rate"]["checks_per_s"],
                          crossover={c["size"]: (round(c["host"]["median_ms"], 3),
                                                 round(c["device"]["median_ms"], 3)) for c in cross},
                          device_faster_from=doc["crossover"]["device_faster_from"])))


if __name__ == "__main__":
    main()
