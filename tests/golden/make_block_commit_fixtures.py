"""The header and the txids of the reference's benchmark block, run in the build container.

    python3 tests/golden/make_block_commit_fixtures.py

Reads depend/bitcoin/src/bench/data/block413567.raw and writes block_commit.json.gz: the 80-byte
header, the transaction count and every transaction's txid as tests/block_model.py computes it (raw
digest bytes, hex).  Data only, as make_block_shape.py's: no transaction travels.  The header's
merkle field is a value the network fixed, so it anchors the model and, through the fixture, the
host route and the kernels: the file is written only if the model's root over these txids equals
header[36:68] and the tree is not mutated.
"""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import block_model as B  # noqa: E402

SRC = "/root/reference/depend/bitcoin/src/bench/data/block413567.raw"
OUT = os.path.join(HERE, "block_commit.json.gz")


def main():
    raw = open(SRC, "rb").read()
    r = B.block_result(raw, 0)
    assert r["status"] == B.OK, r["status"]
    root, mutated = B.merkle_root(r["txids"])
    assert root == raw[36:68] and not mutated, "the model's root is not the header's"
    d = dict(source="block413567.raw (reference bench/data)", header=raw[:80].hex(),
             transactions=r["n_tx"], txids=[t.hex() for t in r["txids"]])
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps(d).encode())
    print(f"{r['n_tx']} txids, root {root.hex()} == header[36:68] -> {OUT}")


if __name__ == "__main__":
    main()
