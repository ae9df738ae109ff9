#!/usr/bin/env python3
"""Measure bcc_block_check_batch on the GPU against its own host route and against
bcc_block_commitments_batch on the same blocks, and write one JSON file.

    python3 tools/block_rules_bench.py [--repeats 15] [--out profiles/block_rules/block_rules_bench.json]

Workload: tools/block_bench.py's blocks (the shape of block 413567, transactions from the C3
workload generator), in its 256-block, one-block and two-block sets.  The generator's coinbase and
outputs carry random values, so most blocks end at a transaction rule; the lanes do the same work
whatever the verdict (no lane stops early), and the statuses are recorded.

Method: one process.  Per set, after one warm-up call of each, three legs alternate `--repeats`
times: bcc_block_check_batch on the device route (bcc_set_host_small_round(0)), the same on the
host route (the threshold above every batch, 16 host threads), and bcc_block_commitments_batch on
the device route, which is what the library could do for these blocks before the rule entries
existed.  A host clock surrounds each synchronous call; medians with minimum and maximum are
reported.  The rule kernels' event times come from bcc_block_rules_last_timing_ms and the hashing
round's from bcc_block_last_timing_ms (BCC_BLOCK_TIMING=1).  Every device result is compared with
the host route's; a mismatch fails the run.  Without a GPU the tool fails: it reports no CPU timing.
`--rehearse` runs the plumbing at a tiny size on the CPU tests' device-less build, prints no time
and writes no file.
"""
import argparse
import ctypes
import json
import os
import sys
import time

os.environ.setdefault("BCC_BLOCK_TIMING", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rust-bitcoinconsensus_amd"), os.path.join(ROOT, "tests"),
                os.path.join(ROOT, "tools")]
import bitcoinconsensus_amd as B  # noqa: E402
import block_bench as BB  # noqa: E402

HEIGHT, CUTOFF = 413567, 1464000000
HOST_THREADS = 16


class Batch:
    """n blocks as both entries take them, each from a buffer of its own."""

    def __init__(self, distinct, n):
        self.n = n
        pick = [distinct[k % len(distinct)] for k in range(n)]
        self.keep = [ctypes.create_string_buffer(raw, len(raw)) for raw, _ in pick]
        self.check = (B.BlockCheckRef * n)()
        self.commit = (B.BlockRef * n)()
        for k, buf in enumerate(self.keep):
            p = ctypes.cast(buf, ctypes.c_char_p)
            self.check[k] = B.BlockCheckRef(p, len(buf), HEIGHT, CUTOFF,
                                            (B.BLOCK_SEGWIT_ACTIVE if pick[k][1] else 0) | B.BLOCK_BIP34_ACTIVE)
            self.commit[k] = B.BlockRef(p, len(buf), pick[k][1], None, 0)
        self.check_res = (B.BlockCheckResult * n)()
        self.commit_res = (B.BlockResult * n)()

    def call_check(self, L):
        t0 = time.perf_counter()
        rc = L.bcc_block_check_batch(self.check, self.n, self.check_res, 0)
        dt = time.perf_counter() - t0
        if rc != 0:
            raise RuntimeError(f"bcc_block_check_batch failed: {rc}")
        return 1e3 * dt

    def call_commit(self, L):
        t0 = time.perf_counter()
        rc = L.bcc_block_commitments_batch(self.commit, self.n, self.commit_res, 0)
        dt = time.perf_counter() - t0
        if rc != 0:
            raise RuntimeError(f"bcc_block_commitments_batch failed: {rc}")
        return 1e3 * dt

    def digest(self):
        return [(r.status, r.tx_index, r.tx_status, r.n_tx, r.sigops, r.stripped_size, r.weight,
                 bytes(r.merkle_root), bytes(r.witness_root)) for r in self.check_res]


def leg(L, distinct, n, repeats):
    b = Batch(distinct, n)
    t = {"check_device": [], "check_host": [], "commitments_device": []}
    rules_ms, round_ms, results, stats = [], [], {}, {}
    for warm in (True, False):
        for _ in range(1 if warm else repeats):
            L.bcc_set_host_small_round(0)
            dt = b.call_check(L)
            st = B.last_block_stats(library=L)
            assert st["host_rounds"] == 0 and st["device_retries"] == 0, st
            if warm:
                results["device"] = b.digest()
            else:
                t["check_device"].append(dt)
                rules_ms.append(B.block_rules_last_timing_ms(library=L))
                round_ms.append(B.block_last_timing_ms(library=L))
                stats = st
            L.bcc_set_host_small_round(BB.HOST_ALL)
            dt = b.call_check(L)
            assert B.last_block_stats(library=L)["device_rounds"] == 0
            if warm:
                results["host"] = b.digest()
            else:
                t["check_host"].append(dt)
            L.bcc_set_host_small_round(0)
            dt = b.call_commit(L)
            assert B.last_block_stats(library=L)["host_rounds"] == 0
            if not warm:
                t["commitments_device"].append(dt)
    if results["device"] != results["host"]:
        raise SystemExit("the device route and the host route disagree")
    for c, k in zip(b.check_res, b.commit_res):
        assert (c.n_tx, bytes(c.merkle_root), bytes(c.witness_root)) == (k.n_tx, bytes(k.merkle_root), bytes(k.witness_root))
    doc = {k + "_ms": BB.spread(v) for k, v in t.items()}
    doc.update(blocks=n, txs=stats["txs"], host_long_txs=stats["host_long_txs"],
               statuses=sorted({r[0] for r in results["device"]}),
               rule_kernels_ms={k: BB.spread([m[k] for m in rules_ms]) for k in rules_ms[0]},
               round_ms={k: BB.spread([m[k] for m in round_ms]) for k in round_ms[0]})
    doc["check_over_commitments"] = doc["check_device_ms"]["median"] / doc["commitments_device_ms"]["median"]
    doc["host_over_device"] = doc["check_host_ms"]["median"] / doc["check_device_ms"]["median"]
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--rehearse", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_rules", "block_rules_bench.json"))
    a = ap.parse_args()
    if a.rehearse:
        import engine_stub
        B._lib = engine_stub.load()
        B.source_hash = lambda: "rehearsal"
    else:  # (torch first: the library then shares the HIP runtime torch has loaded)
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("block_rules_bench.py needs a GPU: it reports no CPU timing")
        torch.cuda.set_device(0)
    L = B._bind_block_rules(B.lib())
    B._bind_consensus(L)
    L.bcc_get_host_threads.restype = ctypes.c_uint
    shp = BB.shape()
    if a.rehearse:
        distinct = [BB.make_block(s, BB.random_txs(s, shp[:40])) for s in range(2)]
        sizes, device = [3, 1, 2], "rehearsal: no timing is reported"
    else:
        B.set_host_threads(HOST_THREADS)
        distinct = [BB.make_block(s, BB.generator_txs(0xB10C0000 + s, shp)) for s in range(a.distinct)]
        sizes, device = [256, 1, 2], torch.cuda.get_device_name(0)
    doc = dict(tool="tools/block_rules_bench.py", source_hash=B.source_hash(), device=device,
               repeats=a.repeats, host_threads=L.bcc_get_host_threads(),
               sets=[leg(L, distinct, n, 2 if a.rehearse else a.repeats) for n in sizes])
    wins = sorted(s["blocks"] for s in doc["sets"] if s["check_device_ms"]["median"] < s["check_host_ms"]["median"])
    doc["device_overtakes_host_at_blocks"] = wins[0] if wins else "never (at the sizes measured)"
    if a.rehearse:
        print("rehearsal ok:", [(s["blocks"], s["txs"], s["statuses"]) for s in doc["sets"]])
        return
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({s["blocks"]: {k: round(s[k], 3) if isinstance(s[k], float) else s[k]["median"]
                                    for k in ("check_device_ms", "check_host_ms", "commitments_device_ms",
                                              "check_over_commitments", "host_over_device")}
                      for s in doc["sets"]}))


if __name__ == "__main__":
    main()
