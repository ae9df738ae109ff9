"""The reference's own recorded header results, as data, run in the build container.

    python3 tests/golden/make_header_fixtures.py <reference>/depend/bitcoin/src

Reads chainparams.cpp (the mainnet genesis block's fields and the hash and merkle root its asserts
fix) and test/pow_tests.cpp (the four CalculateNextWorkRequired cases) and writes
header_cases.json.gz.  Numbers and hex strings only.  The genesis block's proof, 0x100010001, is
the chain work every node reports for block 0.  The file is written only if tests/header_model.py
reproduces every value, so the fixture pins the model and, through it, the host route and the
kernels.
"""
import gzip
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import header_model as M  # noqa: E402

OUT = os.path.join(HERE, "header_cases.json.gz")
MAINNET_LIMIT = 0xffff << 208
TIMESPAN = 14 * 24 * 60 * 60


def main(src):
    cp = open(os.path.join(src, "chainparams.cpp")).read()
    m = re.search(r"CreateGenesisBlock\((\d+), (\d+), (0x[0-9a-f]+), (\d+), 50 \* COIN\)", cp)
    time, nonce, bits, version = int(m[1]), int(m[2]), int(m[3], 16), int(m[4])
    ghash = re.search(r'hashGenesisBlock == uint256S\("0x([0-9a-f]{64})"\)', cp)[1]
    merkle = re.search(r'hashMerkleRoot == uint256S\("0x([0-9a-f]{64})"\)', cp)[1]
    genesis = dict(version=version, merkle_root=merkle, time=time, bits=bits, nonce=nonce, hash=ghash,
                   pow_ok=True, block_proof=0x100010001)
    pt = open(os.path.join(src, "test", "pow_tests.cpp")).read()
    retargets = [dict(first_time=int(a), last_time=int(b), bits=int(c, 16), expected=int(d, 16))
                 for a, b, c, d in re.findall(
                     r"nLastRetargetTime = (\d+);.*?nTime = (\d+);.*?nBits = (0x[0-9a-f]+);.*?"
                     r"CalculateNextWorkRequired\([^;]*?\), (0x[0-9a-f]+)U\)", pt, flags=re.S)]
    assert len(retargets) == 4, retargets

    h = M.header(version, bytes(32), bytes.fromhex(merkle)[::-1], time, bits, nonce)
    assert M.sha256d(h)[::-1].hex() == ghash, "the model's genesis hash"
    assert M.check_pow(M.sha256d(h), bits, MAINNET_LIMIT) and M.block_proof(bits) == 0x100010001
    for r in retargets:
        got = M.next_work(r["bits"], r["last_time"], r["first_time"], TIMESPAN, MAINNET_LIMIT)
        assert got == r["expected"], (r, hex(got))
    d = dict(source="chainparams.cpp CMainParams, test/pow_tests.cpp", genesis=genesis,
             retargets=retargets)
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps(d).encode())
    print(f"genesis {ghash}, {len(retargets)} retarget cases -> {OUT}")


if __name__ == "__main__":
    main(sys.argv[1])
