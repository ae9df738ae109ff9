#!/usr/bin/env python3
"""Measure whole Taproot inputs on the GPU (bcc_taproot_spend_batch) and write one JSON file under
profiles/.

    python3 tools/spend_bench.py [--items 1000000] [--repeats 5] [--sample 50000]
                                 [--out profiles/spend/spend_bench.json]

Workloads, each `--items` spends from host buffers, tiles of a pool of distinct spends (every
spend has a tx of its own; tiling repeats inputs, not work: every item is parsed, interpreted,
hashed and verified on its own):

  key_path  key-path spends, hash types mixed, one in eight with a flipped signature bit;
  mixed     half key path, half script path: depths 0-8, CHECKSIG (CHECKSIGADD)* <m> NUMEQUAL
            leaves with 1-3 signatures, one in eight with a flipped bit, and one item in sixteen a
            spend that reaches no signature check (the fixed class R shapes of
            tests/taproot_spend_cases.py: OP_SUCCESS, limits, mutations, control sizes, ...).

Timing: one warm-up call, then `--repeats` calls, a host clock around each whole synchronous call
(witness rules, interpreter, job building, upload, kernels, download).  Medians and ranges.

Beside it, in the same process on the same device: bcc_taproot_verify_batch over the key-path
workload's own signature checks (the caller has taken the witness apart already), and the ratio.

Agreement on the first `--sample` items of each workload against the reference (oracle/_ref):
items without a signature check against VerifyScript (ref_capture_script), items with signatures
check by check against CheckSchnorrSignature (ref_taproot_check) under the entry point's rule
(tests/taproot_spend_cases.py).  `mismatches` must be 0.
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rust-bitcoinconsensus_amd"), os.path.join(ROOT, "tests")]
import bitcoinconsensus_amd as B  # noqa: E402
import taproot_spend_cases as S  # noqa: E402
from oracle_ctypes import Reference, reference_available  # noqa: E402


def keypath_pool(R, rng, n):
    pool = []
    for k in range(n):
        t = S.s_tx(rng)
        nin = rng.randrange(len(t["vin"]))
        info = S.keypath_spend(R, rng, t, nin, rng.choice(S.HASH_TYPES),
                               tamper="sig_bit" if k % 8 == 7 else None)
        c = S.case_of(t, nin, "s_keypath", checks=info["checks"], arith=info["arith"])
        c["expected"] = S.label_s(R, c)
        pool.append(c)
    return pool


def mixed_pool(R, rng, n):
    pool, fixed = [], []
    for k in range(n):
        if k % 16 == 5:
            if not fixed:
                fixed = [c for c in S.build_class_r(rng) if len(c["tx"]) < 1200]
                rng.shuffle(fixed)
            c = fixed.pop()
            c["expected"] = S.ref_whole(R, c)
            pool.append(c)
            continue
        t = S.s_tx(rng)
        nin = rng.randrange(len(t["vin"]))
        if k % 2 == 0:
            info = S.keypath_spend(R, rng, t, nin, rng.choice(S.HASH_TYPES),
                                   tamper="sig_bit" if k % 8 == 6 else None)
        else:
            nk = rng.randrange(1, 4)
            info = S.signed_spend(R, rng, t, nin, "multi", nk, [True] * nk,
                                  [rng.choice(S.HASH_TYPES) for _ in range(nk)], m=nk,
                                  depth=rng.randrange(0, 9),
                                  tamper=(rng.randrange(nk), "sig_bit") if k % 8 == 7 else None)
        c = S.case_of(t, nin, "s_mixed", checks=info["checks"], arith=info["arith"])
        c["expected"] = S.label_s(R, c)
        pool.append(c)
    return pool


def spend_array(pool, idx):
    arr = (B.TaprootSpend * len(idx))()
    for i, k in enumerate(idx):
        c = pool[k]
        arr[i] = B.TaprootSpend(c["tx"], len(c["tx"]), c["spent"], len(c["spent"]), c["nin"])
    return arr


def spend_call(arr, n, device):
    ret = (ctypes.c_int * n)()
    err = (ctypes.c_int * n)()
    t0 = time.perf_counter()
    rc = B.lib().bcc_taproot_spend_batch(arr, n, ret, err, device)
    dt = time.perf_counter() - t0
    if rc != 0:
        raise RuntimeError(f"bcc_taproot_spend_batch failed: {rc}")
    return dt, ret, err


def check_call(arr, n, device):
    ret = (ctypes.c_int * n)()
    err = (ctypes.c_int * n)()
    t0 = time.perf_counter()
    rc = B.lib().bcc_taproot_verify_batch(arr, n, ret, err, None, device)
    dt = time.perf_counter() - t0
    if rc != 0:
        raise RuntimeError(f"bcc_taproot_verify_batch failed: {rc}")
    return dt, ret, err


def summary(times, n):
    med = statistics.median(times)
    return dict(median_ms=1e3 * med, min_ms=1e3 * min(times), max_ms=1e3 * max(times),
                items_per_s=n / med, calls_ms=[round(1e3 * t, 3) for t in times])


def run_workload(pool, idx, a):
    n = len(idx)
    arr = spend_array(pool, idx)
    spend_call(arr, n, a.device)  # warm-up: tables, buffers, code objects
    runs = [spend_call(arr, n, a.device) for _ in range(a.repeats)]
    ret, err = runs[-1][1], runs[-1][2]
    s = min(a.sample, n)
    mism = [(i, pool[idx[i]]["cls"], (ret[i], err[i]), tuple(pool[idx[i]]["expected"]))
            for i in range(s) if (ret[i], err[i]) != tuple(pool[idx[i]]["expected"])]
    doc = dict(items=n, pool=len(pool), valid=sum(1 for r in ret if r == 1),
               signature_checks=sum(len(pool[k].get("checks", [])) for k in idx),
               tapscript_items_with_checks=sum(1 for k in idx if pool[k].get("checks") and
                                               pool[k]["checks"][0]["leaf"] is not None),
               items_without_checks=sum(1 for k in idx if not pool[k].get("checks")),
               call=summary([r[0] for r in runs], n),
               agreement=dict(sample=s, mismatches=len(mism), first=mism[:5],
                              class_r=sum(1 for i in range(s) if pool[idx[i]]["cls"].startswith("r_")),
                              class_s=sum(1 for i in range(s) if pool[idx[i]]["cls"].startswith("s_"))))
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=int, default=50_000)
    ap.add_argument("--pool", type=int, default=2048)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spend", "spend_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("spend_bench.py needs a GPU: it reports no CPU timing")
    if not reference_available():
        raise SystemExit("spend_bench.py needs the reference build (oracle/_ref): it signs with it")
    B.set_host_small_round(0)
    R = Reference()
    rng = random.Random(0x5BE2D)
    n = a.items
    doc = dict(tool="tools/spend_bench.py", source_hash=B.source_hash(),
               device=torch.cuda.get_device_name(a.device), repeats=a.repeats)
    kp = keypath_pool(R, rng, a.pool)
    idx = [rng.randrange(len(kp)) for _ in range(n)]
    doc["key_path"] = run_workload(kp, idx, a)
    # the same checks through the signature-check entry (the witness already taken apart)
    chk = (B.TaprootCheck * n)()
    for i, k in enumerate(idx):
        c = kp[k]
        q = c["checks"][0]
        chk[i] = B.TaprootCheck(c["tx"], len(c["tx"]), c["spent"], len(c["spent"]), c["nin"], q["sig"],
                                len(q["sig"]), q["pk"], B.SIGVERSION_TAPROOT, None, 0, bytes(32),
                                0xFFFFFFFF)
    check_call(chk, n, a.device)
    cruns = [check_call(chk, n, a.device) for _ in range(a.repeats)]
    doc["key_path_checks_only"] = dict(entry="bcc_taproot_verify_batch", items=n,
                                       call=summary([r[0] for r in cruns], n))
    doc["spend_over_checks_only"] = (doc["key_path"]["call"]["median_ms"] /
                                     doc["key_path_checks_only"]["call"]["median_ms"])
    del chk
    mp = mixed_pool(R, rng, a.pool)
    idx = [rng.randrange(len(mp)) for _ in range(n)]
    doc["mixed"] = run_workload(mp, idx, a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(dict(key_path_items_per_s=doc["key_path"]["call"]["items_per_s"],
                          key_path_median_ms=doc["key_path"]["call"]["median_ms"],
                          checks_only_median_ms=doc["key_path_checks_only"]["call"]["median_ms"],
                          spend_over_checks_only=doc["spend_over_checks_only"],
                          mixed_items_per_s=doc["mixed"]["call"]["items_per_s"],
                          mixed_median_ms=doc["mixed"]["call"]["median_ms"],
                          mismatches=[doc["key_path"]["agreement"]["mismatches"],
                                      doc["mixed"]["agreement"]["mismatches"]])))


if __name__ == "__main__":
    main()
