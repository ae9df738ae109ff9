#!/usr/bin/env python3
"""Measure the block entries (bcc_block_commitments_batch, bcc_merkle_root) on the GPU against the
engine's own host route, and write one JSON file.

    python3 tools/block_bench.py [--repeats 7] [--max-blocks 256] [--out profiles/block/block_bench.json]

Workload: blocks shaped like block 413567 (tests/golden/block413567_shape.json: 1,557 transactions,
the input and output counts of every one), their transactions made by the C3 workload generator
(librbc_bench.so, synthetic keys and signatures of real sizes) behind a coinbase, under a header
that carries the merkle root tests/block_model.py computes.  Where the generator's transactions
carry witness data the coinbase commits to the witness tree and the block is checked as a segwit
block, so both trees run; the output says which.  `--distinct` such blocks are made from
different seeds; a batch of more blocks repeats them, each from a buffer of its own.  Repeating
inputs does not repeat work: every transaction is uploaded and hashed again.

Legs: one block; batches of 1, 2, 4, ... `--max-blocks` blocks; bcc_merkle_root over 2^12 and 2^20
random leaves; the long-chain threshold (bcc_set_host_txhash_blocks) swept on one block and on a
batch.

Method: both routes run in this one process.  After one warm-up call of each route at a size, the
device route (bcc_set_host_small_round(0)) and the host route (the threshold above every batch, on
bcc_get_host_threads() threads) alternate `--repeats` times; a host clock surrounds each synchronous
call, and medians with ranges are reported.  The device route's split comes from the library
(BCC_BLOCK_TIMING=1: event times of the uploads, the two kernels and the downloads; host clocks of
the parse and of the staging).  Every device result is compared with the host route's and the
block's root with the header's; a mismatch fails the run.  Without a GPU the tool fails: it
reports no CPU timing.  `--rehearse` runs the plumbing at a tiny size with transactions of random
bytes on the CPU tests' device-less build of the engine (tests/engine_stub.py), prints no time and
writes no file.
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

os.environ.setdefault("BCC_BLOCK_TIMING", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rust-bitcoinconsensus_amd"), os.path.join(ROOT, "tests")]
import bitcoinconsensus_amd as B  # noqa: E402
import block_model as M  # noqa: E402
import sighash_model as SM  # noqa: E402

HOST_ALL = 1 << 40
THRESHOLDS = (0, 4, 8, 16, 32, 64, 256, 1024)


def shape():
    return [tuple(t) for t in json.load(open(os.path.join(ROOT, "tests", "golden",
                                                          "block413567_shape.json")))["txs"]]


def generator_txs(seed, shp):
    """The distinct transactions of a C3 workload, in order (one item per input: input 0 names it)."""
    w = B.Workload(kind="block", shape=shp, seed=seed)
    try:
        return [w.item(i)[2] for i in range(w.n) if w.item(i)[3] == 0]
    finally:
        w.free()


def random_txs(seed, shp):
    rng = random.Random(seed)
    return [SM.rand_tx(rng, nin, (25,) * nout, sig_lens=[107] * nin) for nin, nout in shp]


def make_block(seed, txs):
    """(raw block, segwit_active): with witness data among the transactions, the coinbase commits
    to the witness tree (BIP141) and the block is a segwit one; else neither."""
    rng = random.Random(seed)
    outs = SM.rand_outs(rng, (25,))
    if not any(M.Tx(t).extended for t in txs):
        return M.make_block(rng, [M.coinbase(rng, outs)] + txs), 0
    nonce = rng.randbytes(32)
    wroot = M.merkle_root([M.ZERO] + [M.Tx(t).wtxid() for t in txs])[0]
    cb = M.coinbase(rng, outs + [M.commit_out(M.sha256d(wroot + nonce))], [[nonce]])
    return M.make_block(rng, [cb] + txs), 1


class Batch:
    """n blocks as the C ABI takes them, each from a buffer of its own."""

    def __init__(self, distinct, n):
        self.n = n
        pick = [distinct[k % len(distinct)] for k in range(n)]
        self.keep = [ctypes.create_string_buffer(raw, len(raw)) for raw, _ in pick]
        self.arr = (B.BlockRef * n)()
        self.txid = []
        for k, buf in enumerate(self.keep):
            cap = 4096
            out = ctypes.create_string_buffer(32 * cap)
            self.txid.append(out)
            self.arr[k] = B.BlockRef(ctypes.cast(buf, ctypes.c_char_p), len(buf), pick[k][1],
                                     ctypes.cast(out, ctypes.c_void_p), cap)
        self.res = (B.BlockResult * n)()
        self.bytes = sum(len(b) for b in self.keep)

    def call(self, L):
        t0 = time.perf_counter()
        rc = L.bcc_block_commitments_batch(self.arr, self.n, self.res, 0)
        dt = time.perf_counter() - t0
        if rc != 0:
            raise RuntimeError(f"bcc_block_commitments_batch failed: {rc}")
        return dt

    def digest(self):
        return ([(r.status, r.n_tx, bytes(r.merkle_root), bytes(r.witness_root)) for r in self.res],
                [t.raw[:32 * self.res[k].n_tx] for k, t in enumerate(self.txid)])


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), calls=[round(x, 4) for x in v])


def ab(L, run, check, repeats):
    """Alternating device / host calls of run(); returns per-route times (ms), the device route's
    stats and split, and checks the two routes' results against each other."""
    out = {"device": [], "host": []}
    split, stats, results = [], {}, {}
    for warm in (True, False):
        for _ in range(1 if warm else repeats):
            for route, small in (("device", 0), ("host", HOST_ALL)):
                L.bcc_set_host_small_round(small)
                dt = run()
                st = B.last_block_stats()
                assert (st["host_rounds"] == 0) == (route == "device") and st["device_retries"] == 0, st
                if warm:
                    results[route] = check()
                    continue
                out[route].append(1e3 * dt)
                stats[route] = st
                if route == "device":
                    split.append(B.block_last_timing_ms())
    L.bcc_set_host_small_round(0)
    if results["device"] != results["host"]:
        raise SystemExit("the device route and the host route disagree")
    doc = dict(device_ms=spread(out["device"]), host_ms=spread(out["host"]), stats=stats["device"],
               device_split_ms={k: spread([s[k] for s in split]) for k in split[0]})
    doc["device_over_host"] = doc["host_ms"]["median"] / doc["device_ms"]["median"]
    return doc


def block_leg(L, distinct, n, repeats):
    b = Batch(distinct, n)
    doc = ab(L, lambda: b.call(L), b.digest, repeats)
    res, _ = b.digest()
    assert all(r[0] == B.BLOCK_OK for r in res), "a block's commitments do not hold"
    txs = doc["stats"]["txs"]
    doc.update(blocks=n, txs=txs, block_bytes=b.bytes, bytes_hashed=doc["stats"]["bytes_hashed"])
    for route in ("device", "host"):
        s = 1e-3 * doc[route + "_ms"]["median"]
        doc[route + "_txs_per_s"] = txs / s
        doc[route + "_bytes_per_s"] = doc["bytes_hashed"] / s
    return doc


def merkle_leg(L, n, repeats):
    leaves = random.Random(n).randbytes(32 * n)
    root = ctypes.create_string_buffer(32)
    mut = ctypes.c_int(0)

    def run():
        t0 = time.perf_counter()
        rc = L.bcc_merkle_root(leaves, n, root, ctypes.byref(mut), 0)
        dt = time.perf_counter() - t0
        if rc != 0:
            raise RuntimeError(f"bcc_merkle_root failed: {rc}")
        return dt
    doc = ab(L, run, lambda: (root.raw, mut.value), repeats)
    doc.update(leaves=n, bytes_hashed=doc["stats"]["bytes_hashed"])
    for route in ("device", "host"):
        doc[route + "_leaves_per_s"] = n / (1e-3 * doc[route + "_ms"]["median"])
    return doc


def threshold_leg(L, distinct, n, repeats):
    """The device route alone with the long-chain threshold swept (0: nothing goes to the host)."""
    b = Batch(distinct, n)
    L.bcc_set_host_small_round(0)
    rows, want = [], None
    for th in THRESHOLDS:
        L.bcc_set_host_txhash_blocks(th)
        b.call(L)
        got = b.digest()
        want = want or got
        assert got == want, th
        t = [1e3 * b.call(L) for _ in range(repeats)]
        rows.append(dict(host_txhash_blocks=th, host_long_txs=B.last_block_stats()["host_long_txs"],
                         call_ms=spread(t), txh_kernel_ms=B.block_last_timing_ms()["txh_kernel"]))
    L.bcc_set_host_txhash_blocks(B.HOST_TXHASH_BLOCKS_DEFAULT)
    return dict(blocks=n, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--max-blocks", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--threshold-blocks", type=int, default=32)
    ap.add_argument("--rehearse", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block", "block_bench.json"))
    a = ap.parse_args()
    if a.rehearse:
        import engine_stub
        B._lib = engine_stub.load()
        B.source_hash = lambda: "rehearsal"
    else:  # (torch first: the library then shares the HIP runtime torch has loaded)
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("block_bench.py needs a GPU: it reports no CPU timing")
        torch.cuda.set_device(0)
    L = B._bind_block(B.lib())
    B._bind_consensus(L)
    L.bcc_get_host_threads.restype = ctypes.c_uint
    shp = shape()
    if a.rehearse:
        shp, sizes, merkle_sizes = shp[:40], [1, 64], [1 << 12]  # (on both sides of the small-round threshold)
        distinct = [make_block(s, random_txs(s, shp)) for s in range(2)]
        device = "rehearsal: no timing is reported"
    else:
        device = torch.cuda.get_device_name(0)
        distinct = [make_block(s, generator_txs(0xB10C0000 + s, shp)) for s in range(a.distinct)]
        sizes = [1 << k for k in range(a.max_blocks.bit_length()) if 1 << k <= a.max_blocks]
        merkle_sizes = [1 << 12, 1 << 20]
    doc = dict(tool="tools/block_bench.py", source_hash=B.source_hash(), device=device,
               repeats=a.repeats, host_threads=L.bcc_get_host_threads(),
               block=dict(transactions=len(shp) + 1, bytes=len(distinct[0][0]), distinct=len(distinct),
                          segwit_active=distinct[0][1],
                          witness_txs=sum(M.Tx(t).extended for t in block_txs(distinct[0][0])) - distinct[0][1],
                          longest_tx_bytes=max(len(t) for t in block_txs(distinct[0][0]))),
               batches=[block_leg(L, distinct, n, a.repeats) for n in sizes],
               merkle=[merkle_leg(L, n, a.repeats) for n in merkle_sizes],
               thresholds=[threshold_leg(L, distinct, n, max(3, a.repeats // 2))
                           for n in sorted({1, min(a.threshold_blocks, sizes[-1])})])
    wins = [b["blocks"] for b in doc["batches"] if b["device_ms"]["median"] < b["host_ms"]["median"]]
    doc["device_overtakes_host_at_blocks"] = wins[0] if wins else "never (at the sizes measured)"
    line = dict(one_block={k: doc["batches"][0][k] for k in ("device_txs_per_s", "host_txs_per_s",
                                                             "device_over_host")},
                largest={k: doc["batches"][-1][k] for k in ("blocks", "device_txs_per_s", "host_txs_per_s",
                                                            "device_bytes_per_s", "host_bytes_per_s",
                                                            "device_over_host")},
                merkle={m["leaves"]: m["device_over_host"] for m in doc["merkle"]},
                device_overtakes_host_at_blocks=doc["device_overtakes_host_at_blocks"])
    if a.rehearse:
        print("rehearsal ok:", json.dumps({k: len(v) if isinstance(v, list) else v
                                           for k, v in doc.items() if k != "block"})[:400])
        return
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(line))


def block_txs(raw):
    r = M.block_result(raw, 1)
    assert r["status"] == M.OK, r["status"]
    pos, out = 80 + len(SM.cs(r["n_tx"])), []
    for _ in range(r["n_tx"]):
        t = M.Tx(raw, pos)
        out.append(t.raw)
        pos = t.end
    return out


if __name__ == "__main__":
    main()
