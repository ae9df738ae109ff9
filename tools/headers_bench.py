#!/usr/bin/env python3
"""Measure bcc_headers_batch on the GPU against the engine's own host route, and write one JSON
file.

    python3 tools/headers_bench.py [--repeats 7] [--out profiles/headers/headers_bench.json]

Workload: one mined low-difficulty chain from a genesis, made here: interval 16 (timespan 16 s,
spacing 1 s), a period's first and last header 17 s apart, pow_limit 0x0f0f0f << 232.  Every 16th
header carries the bits CalculateNextWorkRequired demands (tests/header_model.py computes them:
17/16 of the limit, clamped back to it), so the retarget lanes do their arithmetic; a header takes
about 17 tries.  Sizes: prefixes of that chain of
2,000 (one `headers` message), 2^15, 2^17 and 2^20 headers, and the smaller prefixes of
--crossover-sizes, which locate the size from which the device route is the faster one.

Method: both routes run in this one process.  After one warm-up call of each route at a size, the
device route (bcc_set_host_small_round(0)) and the host route (a threshold above every batch, on
--host-threads threads) alternate `--repeats` times; a host clock surrounds each synchronous call,
and medians with ranges are reported.  The device route's split comes from the library
(BCC_HEADER_TIMING=1: event times of the upload, the two kernels and the download).  Every device
result is compared with the host route's, and every header must pass; a mismatch fails the run.
Without a GPU the tool fails: it reports no CPU timing.  `--rehearse` runs the plumbing at a tiny
size on the CPU tests' device-less build of the engine (tests/engine_stub.py), prints no time and
writes no file.
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import struct
import sys
import time

os.environ.setdefault("BCC_HEADER_TIMING", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rust-bitcoinconsensus_amd"), os.path.join(ROOT, "tests")]
import bitcoinconsensus_amd as B  # noqa: E402
import header_model as M  # noqa: E402

HOST_ALL = 1 << 40
LIMIT = 0x0f0f0f << 232    # times 17 it stays below 2^256, so no retarget product is truncated
INTERVAL, T0 = 16, 1_600_000_000
SIZES = (2000, 1 << 15, 1 << 17, 1 << 20)


def mine_chain(n):
    """n linked headers under the workload's rules, as one byte string; returns it and the tries."""
    out = bytearray()
    prev, bits, tries = bytes(32), M.get_compact(LIMIT), 0
    times = [T0 + i * 17 // 15 for i in range(n)]
    nonces = [struct.pack("<I", k) for k in range(1 << 12)]
    for i in range(n):
        if i and i % INTERVAL == 0:
            bits = M.next_work(bits, times[i - 1], times[i - INTERVAL], INTERVAL, LIMIT)
        target = M.set_compact(bits)[0]
        top = target >> 248
        head = struct.pack("<i32s32sII", 4, prev, i.to_bytes(32, "little"), times[i], bits)
        mid = hashlib.sha256(head[:64])
        for nonce in nonces:
            h = mid.copy()
            h.update(head[64:] + nonce)
            d = hashlib.sha256(h.digest()).digest()
            tries += 1
            if d[31] <= top and int.from_bytes(d, "little") <= target:
                break
        else:
            raise SystemExit("no nonce below 4096")
        out += head + nonce
        prev = d
    return bytes(out), tries


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), calls=[round(x, 4) for x in v])


def leg(L, chain, n, params, repeats):
    """Alternating device / host calls over the first n headers."""
    blob = ctypes.create_string_buffer(chain[:80 * n], 80 * n)
    status = (ctypes.c_int * n)()
    hashes = ctypes.create_string_buffer(32 * n)
    work = ctypes.create_string_buffer(32)

    def run():
        t0 = time.perf_counter()
        rc = L.bcc_headers_batch(blob, n, ctypes.byref(params), None, 0, hashes, status, work, 0)
        dt = time.perf_counter() - t0
        if rc != n:
            raise SystemExit(f"bcc_headers_batch returned {rc} for {n} valid headers")
        return dt

    out = {"device": [], "host": []}
    split, stats, results = [], {}, {}
    for warm in (True, False):
        for _ in range(1 if warm else repeats):
            for route, small in (("device", 0), ("host", HOST_ALL)):
                L.bcc_set_host_small_round(small)
                dt = run()
                st = B.last_header_stats()
                assert (st["host_rounds"] == 0) == (route == "device") and st["device_retries"] == 0, st
                if warm:
                    results[route] = (hashes.raw, bytes(status), work.raw)
                    continue
                out[route].append(1e3 * dt)
                stats[route] = st
                if route == "device":
                    split.append(B.header_last_timing_ms())
    L.bcc_set_host_small_round(0)
    if results["device"] != results["host"]:
        raise SystemExit("the device route and the host route disagree")
    doc = dict(headers=n, device_ms=spread(out["device"]), host_ms=spread(out["host"]),
               device_rounds=stats["device"]["device_rounds"],
               device_split_ms={k: spread([s[k] for s in split]) for k in split[0]},
               upload_bytes=80 * n, download_bytes=36 * n)
    doc["device_over_host"] = doc["host_ms"]["median"] / doc["device_ms"]["median"]
    for route in ("device", "host"):
        doc[route + "_headers_per_s"] = n / (1e-3 * doc[route + "_ms"]["median"])
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--crossover-sizes", default="16,32,64,96,128,192,256,512,1024,4096,8192,16384")
    ap.add_argument("--rehearse", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "headers", "headers_bench.json"))
    a = ap.parse_args()
    if a.rehearse:
        import engine_stub
        B._lib = engine_stub.load()
        B.source_hash = lambda: "rehearsal"
        sizes, device = [100, 3000], "rehearsal: no timing is reported"
    else:  # (torch first: the library then shares the HIP runtime torch has loaded)
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("headers_bench.py needs a GPU: it reports no CPU timing")
        torch.cuda.set_device(0)
        device = torch.cuda.get_device_name(0)
        sizes = sorted(set(SIZES) | {int(s) for s in a.crossover_sizes.split(",") if s})
    L = B._bind_headers(B.lib())
    B._bind_consensus(L)
    L.bcc_get_host_threads.restype = ctypes.c_uint
    L.bcc_set_host_threads(a.host_threads)
    t0 = time.perf_counter()
    chain, tries = mine_chain(sizes[-1])
    mined_s = time.perf_counter() - t0
    params = B.HeaderParams.make(LIMIT, INTERVAL, 1)
    doc = dict(tool="tools/headers_bench.py", source_hash=B.source_hash(), device=device,
               repeats=a.repeats, host_threads=L.bcc_get_host_threads(),
               chain=dict(headers=sizes[-1], interval=INTERVAL, period_seconds=17, pow_limit="0x0f0f0f << 232",
                          tries_per_header=tries / sizes[-1], distinct_bits=len({chain[80 * i + 72: 80 * i + 76]
                                                                                 for i in range(sizes[-1])})),
               sizes=[leg(L, chain, n, params, a.repeats) for n in sizes])
    wins = [s["headers"] for s in doc["sizes"] if s["device_ms"]["median"] < s["host_ms"]["median"]]
    loses = [s["headers"] for s in doc["sizes"] if s["device_ms"]["median"] >= s["host_ms"]["median"]]
    # the smallest measured size from which the device route wins at every larger measured size
    doc["crossover_headers"] = (min(n for n in wins if n > max(loses, default=0))
                                if wins and max(wins) > max(loses, default=0) else "never (at the sizes measured)")
    line = dict(crossover_headers=doc["crossover_headers"],
                sizes={s["headers"]: dict(device_ms=round(s["device_ms"]["median"], 3),
                                          host_ms=round(s["host_ms"]["median"], 3),
                                          device_over_host=round(s["device_over_host"], 2))
                       for s in doc["sizes"]})
    if a.rehearse:
        print("rehearsal ok:", json.dumps(dict(sizes=[s["headers"] for s in doc["sizes"]],
                                               tries_per_header=doc["chain"]["tries_per_header"],
                                               distinct_bits=doc["chain"]["distinct_bits"])))
        return
    doc["chain"]["mined_seconds"] = mined_s
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
