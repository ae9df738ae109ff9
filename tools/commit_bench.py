#!/usr/bin/env python3
"""Measure the BIP341 script-path commitment checks on the GPU (bcc_taproot_commit_batch and
mi_xonly_tweak_check_tuples) and write one JSON file under profiles/.

    python3 tools/commit_bench.py [--items 1000000] [--tuples 4000000] [--repeats 5]
                                  [--ref-sample 50000] [--out profiles/commit/commit_bench.json]

Workload: `--items` commitment checks from host buffers.  They are tiles of a pool of 4096 distinct
spends built with plain Python curve arithmetic (tests/commit_cases.py): the depth mix and the
script lengths are stated in the output, one spend in eight is mutated (wrong parity / key / node
/ script / program), a few have a wrong control size.  `--tuples` rows for the tuple entry are
tiles of 8192 distinct rows (valid, wrong, edge).  Tiling repeats inputs, not work: every lane
hashes and adds on its own.

Timing: one warm-up call per entry, then `--repeats` calls, each a host clock around the whole
synchronous call (row building, upload, kernels, download) and the library's event times per
kernel (BCC_COMMIT_TIMING=1: hash, curve, inversion + compare).  Medians and ranges are reported.

Baseline: the feature is new, so there is none; beside the GPU's rate stands the reference's:
`--ref-sample` of the same items through ref_capture_script (VerifyScript with
P2SH | WITNESS | TAPROOT) on 16 Python threads (the ctypes call releases the lock).  That rate
includes the reference's transaction deserialization and the Python call overhead.  The sample's
(ret, serror) are compared with the GPU's: `mismatches` must be 0.
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

os.environ.setdefault("BCC_COMMIT_TIMING", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "rust-bitcoinconsensus_amd"), os.path.join(ROOT, "tests")]
import bitcoinconsensus_amd as B  # noqa: E402
import commit_cases as C  # noqa: E402
from oracle_ctypes import Reference, reference_available  # noqa: E402

DEPTHS = [0, 1, 1, 2, 2, 3, 3, 4, 5, 6, 8, 10, 13, 16, 21, 32]
LENGTHS = [1, 34, 34, 34, 36, 60, 70, 105, 120, 200, 253, 500]
VERSIONS = [0xC0, 0xC0, 0xC2, 0xFE]


def build_pool(rng, n):
    pool = []
    for k in range(n):
        lv = rng.choice(VERSIONS)
        script = b"\x51" if lv == 0xC0 else rng.randbytes(rng.choice(LENGTHS))
        it = C.make_spend(rng, rng.choice(DEPTHS), script, lv)
        if k % 8 == 7:
            it = C.mutate(rng, it, rng.choice(C.applicable_mutations(it)))
        elif k % 512 == 100:
            it = dict(it, control=it["control"][:-1])
        pool.append(it)
    return pool


def commit_call(arr, n, device):
    ret = (ctypes.c_int * n)()
    err = (ctypes.c_int * n)()
    leaf = ctypes.create_string_buffer(32 * n)
    t0 = time.perf_counter()
    rc = B.lib().bcc_taproot_commit_batch(arr, n, ret, err, leaf, device)
    dt = time.perf_counter() - t0
    if rc != 0:
        raise RuntimeError(f"bcc_taproot_commit_batch failed: {rc}")
    return dt, B.commit_last_kernel_ms(), ret, err


def tuple_call(rows, n, device):
    out = ctypes.create_string_buffer(n)
    t0 = time.perf_counter()
    rc = B.lib().mi_xonly_tweak_check_tuples(rows[0], rows[1], rows[2], rows[3], out, n, device)
    dt = time.perf_counter() - t0
    if rc != 0:
        raise RuntimeError(f"mi_xonly_tweak_check_tuples failed: {rc}")
    return dt, B.commit_last_kernel_ms(), out


def summary(times, n):
    med = statistics.median(times)
    return dict(median_ms=1e3 * med, min_ms=1e3 * min(times), max_ms=1e3 * max(times),
                items_per_s=n / med, calls_ms=[round(1e3 * t, 3) for t in times])


def kernel_summary(ks, n):
    out = {}
    for j, name in enumerate(("hash_kernel", "curve_kernel", "inversion_compare_kernel")):
        v = [k[j] for k in ks]
        out[name] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v),
                         ns_per_item=1e6 * statistics.median(v) / n)
    return out


def reference_rate(pool, idx, threads=16):
    """(items/s, [(ret, serror)]) of VerifyScript over items pool[idx[k]] on `threads` threads."""
    R = Reference()
    L = R.L
    jobs = [(b"\x51\x20" + it["program"], C.spend_tx(it)) for it in pool]
    cap = 4

    def work(part):
        pub, sig, h = (ctypes.create_string_buffer(65 * cap), ctypes.create_string_buffer(80 * cap),
                       ctypes.create_string_buffer(32 * cap))
        pl, sl, vd = (ctypes.c_int * cap)(), (ctypes.c_int * cap)(), (ctypes.c_int * cap)()
        nc, se = ctypes.c_int(0), ctypes.c_int(0)
        out = []
        for i in part:
            spk, tx = jobs[i]
            r = L.ref_capture_script(spk, len(spk), 0, tx, len(tx), 0, C.FLAGS, cap, pub, pl, sig, sl,
                                     h, vd, ctypes.byref(nc), ctypes.byref(se))
            out.append((r, se.value))
        return out

    parts = [idx[k::threads] for k in range(threads)]
    with ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        res = list(ex.map(work, parts))
        dt = time.perf_counter() - t0
    flat = [None] * len(idx)
    for k, part in enumerate(res):
        flat[k::threads] = part
    return len(idx) / dt, flat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--tuples", type=int, default=4_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ref-sample", type=int, default=50_000)
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "commit", "commit_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("commit_bench.py needs a GPU: it reports no CPU timing")
    B.set_host_small_round(0)
    rng = random.Random(0xBE7C4)
    pool = build_pool(rng, a.pool)
    n = a.items
    idx = [rng.randrange(len(pool)) for _ in range(n)]
    keep = [(it["control"], it["script"], it["program"]) for it in pool]
    arr = (B.TaprootCommit * n)()
    for i, k in enumerate(idx):
        c, s, q = keep[k]
        arr[i] = B.TaprootCommit(c, len(c), s, len(s), q)
    commit_call(arr, n, a.device)  # warm-up: tables, buffers, code objects
    runs = [commit_call(arr, n, a.device) for _ in range(a.repeats)]
    ret, err = runs[-1][2], runs[-1][3]
    doc = dict(tool="tools/commit_bench.py", source_hash=B.source_hash(),
               device=torch.cuda.get_device_name(a.device), repeats=a.repeats,
               commit=dict(items=n, pool=len(pool), depth_mix=DEPTHS, script_lengths=LENGTHS,
                           leaf_versions=[hex(v) for v in VERSIONS],
                           mean_depth=sum((len(pool[k]["control"]) - 33) // 32 for k in idx) / n,
                           valid=sum(ret), wrong_control_size=sum(1 for e in err if e == 47),
                           call=summary([r[0] for r in runs], n),
                           kernels=kernel_summary([r[1] for r in runs], n)))
    # the tuple entry
    m = a.tuples
    tpool = C.walk_tuples(rng, 8192 - 64) + (C.edge_tuples(rng) * 3)[:64]
    tidx = [rng.randrange(len(tpool)) for _ in range(m)]
    rows = tuple(b"".join(col) for col in zip(*[(tpool[k][1], bytes([tpool[k][2]]), tpool[k][3], tpool[k][4])
                                                for k in tidx]))
    tuple_call(rows, m, a.device)
    truns = [tuple_call(rows, m, a.device) for _ in range(a.repeats)]
    doc["tuples"] = dict(rows=m, pool=len(tpool), valid=sum(truns[-1][2].raw),
                         call=summary([r[0] for r in truns], m),
                         kernels=kernel_summary([r[1] for r in truns], m))
    # the reference beside it, and agreement on the sample
    if reference_available():
        s = min(a.ref_sample, n)
        rate, ref = reference_rate(pool, idx[:s])
        mism = sum(1 for i in range(s) if (ret[i], err[i]) != ref[i])
        T = C.RefTweak(Reference())
        ts = min(a.ref_sample, m)
        tm = sum(1 for i in range(ts) if truns[-1][2].raw[i] != T.check(*tpool[tidx[i]][1:]))
        doc["reference"] = dict(sample=s, threads=16, items_per_s=rate,
                                note="ref_capture_script (VerifyScript) on 16 Python threads: "
                                     "includes the reference's transaction deserialization and "
                                     "the Python call overhead",
                                mismatches=mism, tuple_sample=ts, tuple_mismatches=tm)
    else:
        doc["reference"] = "not measured: oracle/_ref is not built"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    c, t = doc["commit"], doc["tuples"]
    print(json.dumps(dict(commit_items_per_s=c["call"]["items_per_s"], commit_median_ms=c["call"]["median_ms"],
                          commit_kernel_ms={k: v["median_ms"] for k, v in c["kernels"].items()},
                          tuple_rows_per_s=t["call"]["items_per_s"], tuple_median_ms=t["call"]["median_ms"],
                          tuple_kernel_ms={k: v["median_ms"] for k, v in t["kernels"].items()},
                          reference=doc["reference"])))


if __name__ == "__main__":
    main()
