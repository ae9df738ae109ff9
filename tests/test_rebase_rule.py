"""CPU: the arena layout function (csrc/arena.h) and the rule that makes a part's job records valid
inside a concatenation of parts (csrc/pipeline.h PartBase / TapBase, rebase, part_starts,
taproot_fill_part), through the stand-alone program tests/native/rebase_test.cpp.

The program gets three parts of ECDSA-era checks and three of Taproot checks, chosen here from the
committed goldens (sighash_random.json.gz, taproot_checks.json.gz) so that across the parts every
record kind occurs, the middle part is empty and the last part lacks the LinJob, host-preimage and
key-hash kinds (Taproot: the host-built messages).  It evaluates every part alone and their merge
with the product's host evaluation and requires the digests to agree with each other and with the
reference digests stored in the goldens."""
import gzip
import json
import os
import subprocess

import engine_stub
import sighash_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
SRC = os.path.join(HERE, "native", "rebase_test.cpp")
EXE = os.path.join(HERE, "native", "_build", "rebase_test")


def program():
    engine_stub.load()  # builds engine_host.so: the engine's host code the program links
    csrc = os.path.join(ROOT, "rust-bitcoinconsensus_amd", "csrc")
    deps = [SRC, engine_stub.SO, os.path.join(csrc, "arena.h"), os.path.join(csrc, "pipeline.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        tmp = EXE + f".{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread",
                               "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", tmp, SRC,
                               engine_stub.SO, "-Wl,-rpath," + os.path.dirname(EXE)])
        os.replace(tmp, EXE)
    return EXE


def run(args):
    p = subprocess.run([program()] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def test_layout_function():
    assert "rebase_test ok (layout only)" in run([])


def ecdsa_lines():
    d = json.load(gzip.open(os.path.join(GOLDEN, "sighash_random.json.gz")))
    txs, checks = d["txs"], d["checks"]

    def pick(pred, count, used_tx, distinct=True, key=None):
        out = []
        cand = [c for c in checks if pred(c) and c["tx"] not in used_tx]
        if key:
            cand.sort(key=key)
        for c in cand:
            if distinct and c["tx"] in {o["tx"] for o in out}:
                continue
            out.append(c)
            if len(out) == count:
                break
        assert len(out) == count, (count, len(out))
        used_tx.update(o["tx"] for o in out)
        return out

    base = lambda c: c["hashtype"] & 0x1f
    acp = lambda c: bool(c["hashtype"] & 0x80)
    legacy_all = lambda c: c["sigversion"] == 0 and M.legacy_all_type(c["hashtype"])
    short = lambda c: legacy_all(c) and len(txs[c["tx"]]) // 2 < 300
    longest = lambda c: -len(txs[c["tx"]])
    lin = lambda c: c["sigversion"] == 0 and not M.legacy_all_type(c["hashtype"]) and base(c) != 3
    win = lambda c: c["sigversion"] == 1 and base(c) != 3
    single = lambda c: c["sigversion"] == 1 and base(c) == 3
    single_prevouts = lambda c: single(c) and not acp(c)  # its preimage takes hashPrevouts: a patch

    lines, used = [], set()

    def emit(part, mode, cs):
        for c in cs:
            lines.append(" ".join(["E", str(part), mode, str(c["sigversion"]), str(c["hashtype"]),
                                   str(c["nin"]), str(c["amount"]), txs[c["tx"]], c["code"] or "-",
                                   c["sighash_raw"]]))

    # part 0: every kind; its host-preimage jobs with and without patches; two key-hash records
    dev0 = (pick(short, 2, used) + pick(legacy_all, 1, used, key=longest) + pick(lin, 3, used) +
            pick(win, 2, used) + pick(single, 1, used))
    host0 = pick(single_prevouts, 2, used) + pick(lambda c: c["sigversion"] == 0 and base(c) == 2, 1, used)
    emit(0, "dev", dev0)
    emit(0, "host", host0)
    lines += ["H 0 1", f"H 0 {len(dev0) + len(host0) - 1}"]
    # part 1: nothing.  part 2: templates, BIP143 jobs and SINGLE ones only
    dev2 = (pick(short, 1, used) + pick(legacy_all, 1, used, key=longest) + pick(win, 2, used) +
            pick(single, 2, used))
    emit(2, "dev", dev2)
    return lines


def taproot_lines():
    d = json.load(gzip.open(os.path.join(GOLDEN, "taproot_checks.json.gz")))
    blobs, cases = d["blobs"], [c for c in d["cases"] if c.get("sighash") and c["ret"] in (0, 1)]

    def pick(pred, count, used):
        out = [c for c in cases if pred(c) and id(c) not in used][:count]
        assert len(out) == count, (count, len(out))
        used.update(id(c) for c in out)
        return out

    # a SigMsg the program can write by hand: no annex, SIGHASH_DEFAULT or SIGHASH_ALL
    plain = lambda c: c["annex"] is None and (len(c["sig"]) == 128 or c["sig"].endswith("01"))
    lines, used = [], set()

    def emit(part, mode, cs):
        for c in cs:
            lines.append(" ".join(["T", str(part), mode, str(c["sigversion"]), str(c["nin"]),
                                   str(c["codesep"]), blobs[c["tx"]], blobs[c["spent"]], c["sig"],
                                   c["pk"], c["annex"] or "-", c["tapleaf"] or "-", c["sighash"],
                                   str(c["ret"])]))

    host0 = (pick(lambda c: plain(c) and c["cls"] == "valid" and c["sigversion"] == 0, 2, used) +
             pick(lambda c: plain(c) and c["cls"] == "valid" and c["sigversion"] == 1, 1, used) +
             pick(lambda c: plain(c) and c["cls"] == "sig_flip", 1, used))
    dev0 = (pick(lambda c: c["cls"] == "valid" and c["annex"], 2, used) +
            pick(lambda c: c["cls"] == "many_inputs", 2, used) +
            pick(lambda c: c["cls"] == "output" and c["ret"] == 1 and c["sigversion"] == 1, 1, used) +
            pick(lambda c: c["cls"] == "pk_flip", 1, used))
    # interleaved: a host-built row between device-built ones and the other way round
    mixed = [x for pair in zip(dev0, host0 + [None] * (len(dev0) - len(host0))) for x in pair if x]
    for c in mixed:
        emit(0, "dev" if any(c is x for x in dev0) else "host", [c])
    dev2 = (pick(lambda c: c["cls"] == "valid" and c["sigversion"] == 1, 2, used) +
            pick(lambda c: c["cls"] == "output" and c["ret"] == 1 and c["annex"], 2, used) +
            pick(lambda c: c["cls"] == "sig_flip" and c["annex"], 1, used))
    emit(2, "dev", dev2)
    return lines


def test_parts_alone_merged_and_reference_digests_agree(tmp_path):
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(ecdsa_lines() + taproot_lines()) + "\n")
    assert "rebase_test ok" in run([str(path)])
