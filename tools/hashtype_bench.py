#!/usr/bin/env python3
"""What bcc_set_device_hashtypes costs and saves on a block whose signers chose NONE / SINGLE.

Workload: the block-413567-shaped transaction set of bench.py's C3 (tests/golden/
block413567_shape.json: 1,556 transactions, 4,886 inputs, one of 442 inputs), turned into sighash
checks: one per P2PKH / P2WPKH input, two per 2-of-3 multisig input, with the scriptCode the
interpreter would pass.  Every LEGACY check's hash type is then rewritten in turn to 2, 3, 0x82
and 0x83 (the BIP143 checks keep SIGHASH_ALL), and each variant runs through
bcc_debug_sighash_timed -- the whole call from host buffers: job building, staging, upload, the
sighash kernels, the copy back -- with the switch off (the host preimage path, the parent's code)
and on, interleaved in one process: off, on, off, on, ... so that clock and thermal drift hit both
alike.  The first pair of every variant is a warm-up and is dropped.

Per variant and setting: the median over --reps calls of the host job-build time, the staging
time, the uploaded bytes, the sighash kernels' event time and the whole call; and the number of
digests that differ between the two settings (must be 0) and from tests/sighash_model.py on a
sample.  Results: profiles/hashtypes/<name>.json and .txt.

    python3 tools/hashtype_bench.py [--reps 7] [--device 0] [--name block413567]
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
import sighash_model as M  # noqa: E402

HASH_TYPES = (2, 3, 0x82, 0x83)


def pushes(script):
    """The pushed items of a push-only script."""
    out, i = [], 0
    while i < len(script):
        op = script[i]
        i += 1
        if op == 0:
            n = 0
        elif op < 0x4c:
            n = op
        elif op == 0x4c:
            n, i = script[i], i + 1
        elif op == 0x4d:
            n, i = script[i] | script[i + 1] << 8, i + 2
        else:
            raise ValueError(hex(op))
        out.append(script[i:i + n])
        i += n
    return out


def block_checks(seed, device):
    """[(tx, scriptCode, n_in, hashtype, amount, sigversion)] of the C3 block, in tx order; the
    checks of one transaction share its bytes object."""
    shape = [tuple(t) for t in json.load(open(os.path.join(
        ROOT, "tests", "golden", "block413567_shape.json")))["txs"]]
    wl = B.Workload(kind="block", shape=shape, seed=seed, device=device)
    checks, last = [], None
    for i in range(wl.n):
        spk, amount, tx, nin = wl.item(i)
        if last is not None and tx == last:
            tx = last
        last = tx
        if len(spk) == 25 and spk[:3] == b"\x76\xa9\x14":  # P2PKH
            checks.append((tx, spk, nin, 1, 0, 0))
        elif len(spk) == 22 and spk[:2] == b"\x00\x14":  # P2WPKH
            checks.append((tx, b"\x76\xa9\x14" + spk[2:] + b"\x88\xac", nin, 1, amount, 1))
        elif len(spk) == 23 and spk[0] == 0xa9:  # P2SH 2-of-3 multisig: one check per signature
            redeem = pushes(M.parse_tx(tx)["vin"][nin][1])[-1]
            checks += [(tx, redeem, nin, 1, 0, 0)] * 2
        else:
            raise ValueError(spk.hex())
    wl.free()
    return checks


def rewritten(checks, ht):
    return [(tx, code, nin, ht if sv == 0 else h, amount, sv)
            for tx, code, nin, h, amount, sv in checks]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED0003)
    ap.add_argument("--name", default="block413567")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hashtypes"))
    a = ap.parse_args()
    base = block_checks(a.seed, a.device)
    legacy = sum(1 for c in base if c[5] == 0)
    result = dict(workload="block413567-shaped C3 set as sighash checks", checks=len(base),
                  legacy_checks=legacy, bip143_checks=len(base) - legacy, reps=a.reps,
                  method="bcc_debug_sighash_timed, switch off / on interleaved in one process, "
                         "first pair dropped, medians", variants=[])
    lines = []
    for ht in HASH_TYPES:
        checks = rewritten(base, ht)
        runs = {0: [], 1: []}
        kinds, digests = {}, {}
        for rep in range(a.reps + 1):
            for on in (0, 1):
                B.set_device_hashtypes(on)
                t0 = time.perf_counter()
                got, t = B.debug_sighash_timed(checks, a.device)
                t["call_seconds"] = time.perf_counter() - t0
                kinds[on] = B.last_sighash_kinds()
                digests[on] = got
                if rep:
                    runs[on].append(t)
        B.set_device_hashtypes(0)
        differ = sum(1 for x, y in zip(digests[0], digests[1]) if x != y)
        step = max(1, len(checks) // 300)
        model_bad = sum(1 for c, g in list(zip(checks, digests[1]))[::step] if M.sighash(*c) != g)
        v = dict(hashtype=ht, digests_differing=differ, model_sample=len(checks[::step]),
                 model_sample_differing=model_bad)
        for on in (0, 1):
            med = {k: statistics.median(r[k] for r in runs[on]) for k in runs[on][0]}
            v["on" if on else "off"] = dict(med, kinds=kinds[on],
                                            spread_total=[min(r["total_seconds"] for r in runs[on]),
                                                          max(r["total_seconds"] for r in runs[on])])
        off, on_ = v["off"], v["on"]
        v["ratio_total_off_over_on"] = off["total_seconds"] / on_["total_seconds"]
        v["ratio_build_off_over_on"] = off["build_seconds"] / on_["build_seconds"]
        v["ratio_upload_off_over_on"] = off["upload_bytes"] / on_["upload_bytes"]
        v["ratio_kernel_off_over_on"] = off["kernel_seconds"] / on_["kernel_seconds"]
        result["variants"].append(v)
        lines.append(f"hashtype {ht:#04x}: {differ} digests differ between the settings, "
                     f"{model_bad} of {v['model_sample']} sampled differ from the model")
        for name, r in (("off", off), ("on ", on_)):
            lines.append(f"  {name} build {r['build_seconds'] * 1e3:8.3f} ms  stage "
                         f"{r['stage_seconds'] * 1e3:7.3f} ms  upload {r['upload_bytes']:>10} B  "
                         f"kernels {r['kernel_seconds'] * 1e3:7.3f} ms  whole call "
                         f"{r['total_seconds'] * 1e3:8.3f} ms  {r['kinds']}")
        lines.append(f"  off / on: whole call {v['ratio_total_off_over_on']:.2f}x, build "
                     f"{v['ratio_build_off_over_on']:.2f}x, upload {v['ratio_upload_off_over_on']:.2f}x, "
                     f"kernels {v['ratio_kernel_off_over_on']:.2f}x")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.name + ".json"), "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    head = (f"{result['workload']}: {result['checks']} checks ({legacy} legacy rewritten, "
            f"{len(base) - legacy} BIP143 SIGHASH_ALL); {result['method']}; {a.reps} reps")
    with open(os.path.join(a.out, a.name + ".txt"), "w") as fh:
        fh.write("\n".join([head] + lines) + "\n")
    print("\n".join([head] + lines))
    return 1 if any(v["digests_differing"] or v["model_sample_differing"] for v in result["variants"]) else 0


if __name__ == "__main__":
    sys.exit(main())
