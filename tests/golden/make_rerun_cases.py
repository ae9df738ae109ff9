"""Verdict-dependent spends labelled by the reference (run where oracle/_ref is built).

    python3 tests/golden/make_rerun_cases.py

The inputs are constructed by tests/rerun_cases.py (build_all): signatures by the reference's
libsecp256k1 (Reference.sign) over the oracle's signature hash.  Every expected value -- (ret, err)
of verify_script_with_amount and the executed checks of capture_script -- is what the REFERENCE
library (oracle/_ref) returns for exactly those inputs under each of the three flag sets.
Output: rerun_cases.json.gz (layout in tests/rerun_cases.py); regenerates byte for byte.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rerun_cases  # noqa: E402
from oracle_ctypes import Oracle, Reference  # noqa: E402


def main():
    d = rerun_cases.build_all(Reference(), Oracle())
    raw = rerun_cases.dumps(d)
    with open(rerun_cases.GOLDEN, "wb") as fh:
        fh.write(raw)
    cs = d["cases"]
    hist = {}
    for c in cs:
        hist[c["rounds_min"]] = hist.get(c["rounds_min"], 0) + 1
    print(f"rerun_cases: {len(cs)} cases ({sum(c['ret'] for c in cs)} valid), {len(d['blobs'])} blobs, "
          f"{len(d['sighashes'])} sighashes, {len(raw)} bytes; rounds_min {sorted(hist.items())}")
    for fam in rerun_cases.FAMILIES:
        print(" ", fam, sum(c["family"] == fam for c in cs))


if __name__ == "__main__":
    main()
