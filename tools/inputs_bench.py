#!/usr/bin/env python3
"""Measure bcc_verify_inputs_batch (any input against its spent outputs, v1 and older kinds in one
call) beside the two entries it routes to, and write one JSON file under profiles/.

    python3 tools/inputs_bench.py [--sizes 1000000,13170] [--repeats 5] [--sample 50000]
                                  [--out profiles/inputs/inputs_bench.json]

Workload: a pool of `--pool` (2,048) distinct mixed transactions of 1-3 inputs from a seed, signed
through the reference (oracle/_ref; tests/mixed_input_cases.py): about 50 % P2WPKH, 10 % P2PKH /
P2SH-P2WPKH / 2-of-3 P2WSH, 30 % Taproot key path, 10 % Taproot script path; one input in eight is
tampered.  The pool's transactions, every input an item and a transaction's inputs adjacent, are
tiled to each size (tiling repeats inputs, not work: every item is routed, parsed, interpreted,
hashed and verified on its own).

Timing: one warm-up call of each of the three entries, then `--repeats` rounds, each round timing,
in this order, the unified call (all items), bitcoinconsensus_verify_batch on the pre-split non-v1
subset and bcc_taproot_spend_batch on the pre-split v1 subset: a host clock around each whole
synchronous call.  Medians and ranges; `unified_over_split` is the unified median over the sum of
the two split medians, `routing_share` the unified call's route_seconds over its total_seconds
(bcc_last_inputs_stats of the median call).

Agreement: the unified answers equal the split calls' on every item (`split_mismatches`), and the
reference's labels on the first `--sample` items (`label_mismatches`).  Both must be 0.
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rust-bitcoinconsensus_amd"), os.path.join(ROOT, "tests")]
import bitcoinconsensus_amd as B  # noqa: E402
import mixed_input_cases as M  # noqa: E402
from oracle_ctypes import Oracle, Reference, reference_available  # noqa: E402

# kinds in M.KINDS order: p2pkh, p2wpkh, p2sh_p2wpkh, p2wsh_2of3, p2sh_2of3, tr_key, tr_script
WEIGHTS = [1 / 30, 0.5, 1 / 30, 1 / 30, 0, 0.3, 0.1]
FLAGS = M.ALL | M.TAPROOT
INPUT_DT = np.dtype(dict(names=["tx", "tx_len", "spent", "spent_len", "n_in"],
                         formats=["u8", "u4", "u8", "u4", "u4"], offsets=[0, 8, 16, 24, 28],
                         itemsize=ctypes.sizeof(B.InputItem)))
BATCH_DT = np.dtype(dict(names=["spk", "spk_len", "amount", "tx", "tx_len", "n_in"],
                         formats=["u8", "u4", "i8", "u8", "u4", "u4"], offsets=[0, 8, 16, 24, 32, 36],
                         itemsize=ctypes.sizeof(B.BatchItem)))


def addr(b):
    """The address of a bytes object's buffer (the caller keeps the object alive)."""
    return ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value or 0


def spent_out(spent, nin):
    """(amount, script) of output nin of a spent-outputs blob (short compact sizes)."""
    o = 1
    for k in range(nin + 1):
        ln = spent[o + 8]
        if k == nin:
            return int.from_bytes(spent[o:o + 8], "little", signed=True), spent[o + 9:o + 9 + ln]
        o += 9 + ln
    raise IndexError(nin)


def build_pool(n_txs, seed):
    """(txs, per-input records): the labelled pool and one InputItem / BatchItem record per input."""
    R, O, rng = Reference(), Oracle(), random.Random(seed)
    txs, keep = [], []
    while len(txs) < n_txs:
        n = rng.randrange(1, 4)
        kinds = rng.choices(M.KINDS, WEIGHTS, k=n)
        tampers = [rng.choice(M.TAMPERS) if rng.random() < 0.125 else None for _ in range(n)]
        txs.append(M.label_mixed(R, M.build_mixed_tx(R, O, rng, kinds, tampers)))
    n_in = sum(len(t["inputs"]) for t in txs)
    inp, bat = np.zeros(n_in, INPUT_DT), np.zeros(n_in, BATCH_DT)
    v1, ret, first = np.zeros(n_in, bool), np.zeros(n_in, np.int32), []
    k = 0
    for t in txs:
        first.append(k)
        for nin, i in enumerate(t["inputs"]):
            amount, spk = spent_out(t["spent"], nin)
            keep.append(spk)
            inp[k] = (addr(t["tx"]), len(t["tx"]), addr(t["spent"]), len(t["spent"]), nin)
            bat[k] = (addr(spk), len(spk), amount, addr(t["tx"]), len(t["tx"]), nin)
            v1[k], ret[k] = i["kind"] in M.V1_KINDS, i["ret"]
            k += 1
    first.append(k)
    return txs, dict(inp=inp, bat=bat, v1=v1, ret=ret, first=np.array(first), keep=keep)


def tile(P, n, rng):
    """Pool-input indices of n items: whole transactions in random order, the last one cut."""
    first = P["first"]
    out, total = [], 0
    while total < n:
        t = rng.randrange(len(first) - 1)
        out.append(np.arange(first[t], first[t + 1]))
        total += first[t + 1] - first[t]
    return np.concatenate(out)[:n]


def ptr(a, T):
    return ctypes.cast(a.ctypes.data, ctypes.POINTER(T))


def call_unified(items, n):
    ret, err = np.zeros(n, np.int32), np.zeros(n, np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    L = B._bind_inputs(B.lib())
    t0 = time.perf_counter()
    rc = L.bcc_verify_inputs_batch(ptr(items, B.InputItem), n, FLAGS, ctypes.cast(ret.ctypes.data, ip),
                                   ctypes.cast(err.ctypes.data, ip))
    dt = time.perf_counter() - t0
    if rc < 0:
        raise RuntimeError("bcc_verify_inputs_batch failed")
    return dt, ret, err, B.last_inputs_stats()


def call_ecdsa(items, n):
    ret, err = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    t0 = time.perf_counter()
    rc = B.lib().bitcoinconsensus_verify_batch(ptr(items, B.BatchItem), n, M.ALL,
                                               ctypes.cast(ret.ctypes.data, ip),
                                               ctypes.cast(err.ctypes.data, ip))
    dt = time.perf_counter() - t0
    if rc < 0:
        raise RuntimeError("bitcoinconsensus_verify_batch failed")
    return dt, ret[:n], err[:n]


def call_taproot(items, n):
    ret, err = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    t0 = time.perf_counter()
    rc = B.lib().bcc_taproot_spend_batch(ptr(items, B.TaprootSpend), n, ctypes.cast(ret.ctypes.data, ip),
                                         ctypes.cast(err.ctypes.data, ip), -1)
    dt = time.perf_counter() - t0
    if rc != 0:
        raise RuntimeError("bcc_taproot_spend_batch failed")
    return dt, ret[:n], err[:n]


def summary(times, n):
    med = statistics.median(times)
    return dict(median_ms=1e3 * med, min_ms=1e3 * min(times), max_ms=1e3 * max(times),
                items_per_s=n / med if med else None, calls_ms=[round(1e3 * t, 3) for t in times])


def run_size(P, n, a):
    idx = tile(P, n, random.Random(n))
    v1 = P["v1"][idx]
    items = np.ascontiguousarray(P["inp"][idx])
    ec_items = np.ascontiguousarray(P["bat"][idx[~v1]])
    tp_items = np.ascontiguousarray(P["inp"][idx[v1]])
    ne, nt = len(ec_items), len(tp_items)
    call_unified(items, n), call_ecdsa(ec_items, ne), call_taproot(tp_items, nt)  # warm-up
    uni, ec, tp = [], [], []
    for _ in range(a.repeats):  # alternating, in one process
        uni.append(call_unified(items, n))
        ec.append(call_ecdsa(ec_items, ne))
        tp.append(call_taproot(tp_items, nt))
    ret, err = uni[-1][1], uni[-1][2]
    split_bad = int(np.count_nonzero(ret[~v1] != ec[-1][1]) + np.count_nonzero(err[~v1] != ec[-1][2]) +
                    np.count_nonzero(ret[v1] != (tp[-1][1] == 1)) + np.count_nonzero(err[v1] != 0))
    s = min(a.sample, n)
    label_bad = np.flatnonzero((ret[:s] != P["ret"][idx[:s]]) | (err[:s] != 0))
    times = [r[0] for r in uni]
    med_call = sorted(uni, key=lambda r: r[0])[len(uni) // 2]
    st = med_call[3]
    split_sum = statistics.median(r[0] for r in ec) + statistics.median(r[0] for r in tp)
    return dict(items=n, v1_items=nt, non_v1_items=ne, valid=int(np.count_nonzero(ret == 1)),
                unified=summary(times, n), split_ecdsa=summary([r[0] for r in ec], ne),
                split_taproot=summary([r[0] for r in tp], nt), split_sum_median_ms=1e3 * split_sum,
                unified_over_split=statistics.median(times) / split_sum,
                stats_of_median_call=st, routing_share=st["route_seconds"] / st["total_seconds"],
                agreement=dict(split_mismatches=split_bad, label_sample=s,
                               label_mismatches=int(len(label_bad)),
                               first=[int(i) for i in label_bad[:5]]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,13170")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=int, default=50_000)
    ap.add_argument("--pool", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inputs", "inputs_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("inputs_bench.py needs a GPU: it reports no CPU timing")
    if not reference_available():
        raise SystemExit("inputs_bench.py needs the reference build (oracle/_ref): it signs with it")
    B.set_host_small_round(0)
    txs, P = build_pool(a.pool, 0x1A9075B)
    ins = [i for t in txs for i in t["inputs"]]
    doc = dict(tool="tools/inputs_bench.py", source_hash=B.source_hash(),
               device=torch.cuda.get_device_name(0), repeats=a.repeats, host_threads=B.host_threads(),
               pool=dict(txs=len(txs), inputs=len(ins), valid=sum(i["ret"] for i in ins),
                         kinds={k: sum(i["kind"] == k for i in ins) for k in M.KINDS}),
               sizes=[run_size(P, int(s), a) for s in a.sizes.split(",")])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps([dict(items=d["items"], unified_ms=d["unified"]["median_ms"],
                           split_ecdsa_ms=d["split_ecdsa"]["median_ms"],
                           split_taproot_ms=d["split_taproot"]["median_ms"],
                           unified_over_split=d["unified_over_split"], routing_share=d["routing_share"],
                           mismatches=[d["agreement"]["split_mismatches"],
                                       d["agreement"]["label_mismatches"]]) for d in doc["sizes"]]))


if __name__ == "__main__":
    main()
