"""The reference's transaction test vectors, as data, with the model's verdicts, run in the build
container.

    python3 tests/golden/make_tx_check_fixtures.py <reference>/depend/bitcoin/src

Reads the data files test/data/tx_valid.json and test/data/tx_invalid.json (rows of [prevouts,
serialized transaction, flags]; comment rows have one string) and writes tx_check_cases.json.gz:
per transaction its hex, which file it came from, whether it stands under the "Tests for
CheckTransaction()" comment of tx_invalid.json, and tests/block_rules_model.py's result.  Two pins
make it more than the model talking to itself, and the file is written only if both hold: every
transaction of tx_valid.json passes CheckTransaction, and the rows under that comment fail with the
reject reason their own comments name, in order.
"""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import block_rules_model as M  # noqa: E402

OUT = os.path.join(HERE, "tx_check_cases.json.gz")
SECTION = "Tests for CheckTransaction()"
# "No outputs", "Negative output", "MAX_MONEY + 1 output", "MAX_MONEY output + 1 output",
# "Duplicate inputs", "Coinbase of size 1", "Coinbase of size 101", "Null txin ..." (two rows)
SECTION_CODES = [M.VOUT_EMPTY, M.VOUT_NEGATIVE, M.VOUT_TOOLARGE, M.TXOUTTOTAL_TOOLARGE,
                 M.INPUTS_DUPLICATE, M.CB_LENGTH, M.CB_LENGTH, M.PREVOUT_NULL, M.PREVOUT_NULL]


def rows_of(path, name):
    out, in_section = [], False
    for row in json.load(open(path)):
        if len(row) == 1:
            if row[0] == SECTION and name == "tx_invalid.json":
                in_section = True
            elif in_section and row[0].startswith("Same as the transactions in valid"):
                in_section = False
            continue
        raw = bytes.fromhex(row[1])
        out.append(dict(tx=raw.hex(), source=name, check_transaction_section=in_section,
                        result=M.tx_result(raw)))
    return out


def main(src):
    data = os.path.join(src, "test", "data")
    valid = rows_of(os.path.join(data, "tx_valid.json"), "tx_valid.json")
    invalid = rows_of(os.path.join(data, "tx_invalid.json"), "tx_invalid.json")
    assert len(valid) > 100 and len(invalid) > 80
    assert all(r["result"]["status"] == M.TX_OK for r in valid), "a tx_valid.json row fails"
    section = [r["result"]["status"] for r in invalid if r["check_transaction_section"]]
    assert section == SECTION_CODES, section
    d = dict(source="test/data/tx_valid.json, test/data/tx_invalid.json", cases=valid + invalid)
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(json.dumps(d, sort_keys=True).encode())
    print(f"{OUT}: {len(valid)} + {len(invalid)} transactions, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
