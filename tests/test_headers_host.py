"""CPU: bcc_headers_batch and mi_pow_check_tuples in the device-less engine build
(tests/engine_stub.py), where a device round is the host evaluation behind the device seam: the
argument rules, the round cuts and what a round's first headers get from before it, the chain
work, the failure rules and the statistics, every case of tests/header_cases.py against
tests/header_model.py; the model itself against the reference's recorded results
(tests/golden/header_cases.json.gz); and the kernels' lane code as a stand-alone program
(tests/native/header_host.cpp), plainly and under the address and undefined-behaviour sanitizers.
The -m gpu twin is test_headers_gpu.py."""
import gzip
import json
import os
import random
import subprocess

import pytest

import bitcoinconsensus_amd as B
import engine_stub
import header_cases as K
import header_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rust-bitcoinconsensus_amd", "csrc")
MAINNET_LIMIT = 0xffff << 208
MAINNET_SPAN = 14 * 24 * 60 * 60


@pytest.fixture(scope="module")
def L():
    return K.bind(engine_stub.load())


@pytest.fixture(scope="module")
def golden():
    with gzip.open(os.path.join(HERE, "golden", "header_cases.json.gz")) as f:
        return json.load(f)


def genesis_header(g):
    return M.header(g["version"], bytes(32), bytes.fromhex(g["merkle_root"])[::-1], g["time"], g["bits"],
                    g["nonce"])


def test_model_reproduces_the_reference_results(golden):
    g = golden["genesis"]
    h = genesis_header(g)
    assert M.sha256d(h)[::-1].hex() == g["hash"] == "000000000019d6689c085ae165831e934ff763ae46a2a6c172b3f1b60a8ce26f"
    assert M.check_pow(M.sha256d(h), g["bits"], MAINNET_LIMIT) is g["pow_ok"] is True
    assert M.block_proof(g["bits"]) == g["block_proof"] == 0x100010001
    assert len(golden["retargets"]) == 4
    for r in golden["retargets"]:
        assert M.next_work(r["bits"], r["last_time"], r["first_time"], MAINNET_SPAN, MAINNET_LIMIT) == r["expected"]
    assert bytes(B.MAINNET.pow_limit) == MAINNET_LIMIT.to_bytes(32, "little")
    assert (B.MAINNET.pow_target_timespan, B.MAINNET.pow_target_spacing) == (1209600, 600)
    assert (B.MAINNET.bip34_height, B.MAINNET.bip66_height, B.MAINNET.bip65_height) == (227931, 363725, 388381)


def test_reference_results_through_the_engine(L, golden):
    """The mainnet genesis header under B.MAINNET: its hash, its proof of work and its block proof.
    (The recorded retargets reach the engine's code through the lane program below: a header at
    their difficulty cannot be mined here, and without its proof of work no later rule is reached.)"""
    g = golden["genesis"]
    for route, kw in K.ROUTES:
        with K.settings(L, **kw):
            got = B.check_headers([genesis_header(g)], library=L)
            assert got["first_invalid"] == 1 and got["status"] == [B.HEADER_OK]
            assert got["hashes"][0][::-1].hex() == g["hash"] and got["chain_work"] == g["block_proof"]
            bad = genesis_header(dict(g, nonce=g["nonce"] + 1))
            got = B.check_headers([bad], library=L)
            assert got["first_invalid"] == 0 and got["status"] == [B.HEADER_HIGH_HASH] and got["chain_work"] == 0


def test_lane_geometry(L):
    K.check_lane_geometry(L)


def test_device_list_equals_the_single_device(L):
    K.check_device_list(L, lambda devs: engine_stub.set_devices(L, devs))


def test_compact_targets(L):
    K.check_compact_targets(L)


def test_retargets(L):
    K.check_retargets(L)


def test_times(L):
    K.check_times(L)


def test_versions(L):
    K.check_versions(L)


def test_linkage(L):
    K.check_linkage(L)


def test_order_and_work(L):
    K.check_order_and_work(L)


def test_injected_faults_retry_fall_back_and_report(L):
    assert K.fault_sequence(L)


def test_small_round_threshold_routes_to_the_host(L):
    """With bcc_set_host_small_round at its default the entries' own thresholds decide: a batch at
    the threshold runs on the host, one above it is a device round (128 headers, 2,048 rows)."""
    base = list(K.base_chain())
    rows = K.pow_rows()[:2049]
    blob, bits = b"".join(h for h, _ in rows), [b for _, b in rows]
    with K.settings(L, small_round=B.HOST_SMALL_ROUND_DEFAULT):
        for n, host in ((128, 1), (129, 0)):
            assert K.run(L, base[:n], K.PARAMS)["first_invalid"] == n
            st = B.last_header_stats(library=L)
            assert (st["host_rounds"], st["device_rounds"], st["headers"]) == (host, 1 - host, n), st
        for n, host in ((2048, 1), (2049, 0)):
            B.pow_check_tuples(blob[:32 * n], bits[:n], K.LOW_LIMIT, library=L)
            st = B.last_header_stats(library=L)
            assert (st["host_rounds"], st["device_rounds"], st["headers"]) == (host, 1 - host, n), st
    with K.settings(L, small_round=1000):  # a caller's larger threshold raises both
        K.run(L, base, K.PARAMS)
        assert B.last_header_stats(library=L)["host_rounds"] == 1


def model_context(params, anchor):
    """The context record of a round that starts at header 0, as the lane program reads it."""
    interval = params["timespan"] // params["spacing"]
    lim = "%064x" % params["pow_limit"]
    gates = [params.get(k, 0) for k in ("bip34", "bip66", "bip65")]
    if anchor is None:
        tail = [0, 1, 0, bytes(32).hex(), 0, 0]
    else:
        tail = [anchor["height"] + 1, 0, anchor["bits"], anchor["hash"].hex(), anchor["period_first_time"],
                len(anchor["times"])] + list(anchor["times"])
    return [lim, params["timespan"], interval, int(params.get("no_retargeting", False))] + gates, tail


def lane_rows(golden):
    rows = []
    g = golden["genesis"]
    h = genesis_header(g)
    rows.append(f"hash {h.hex()} {bytes.fromhex(g['hash'])[::-1].hex()}")
    rows.append(f"pow {M.sha256d(h).hex()} {g['bits']} {MAINNET_LIMIT:064x} 1")
    for r in golden["retargets"]:
        rows.append(f"next {r['bits']} {r['last_time']} {r['first_time']} {MAINNET_SPAN} {MAINNET_LIMIT:064x} 0 "
                    f"{r['expected']}")
    rng = random.Random(K.SEED + 8)
    for _ in range(300):  # mainnet-sized factors: 32-bit multipliers and divisors
        span = rng.choice((MAINNET_SPAN, (1 << 30) - 1, rng.randrange(4, 1 << 30)))
        bits = rng.choice((0x1d00ffff, 0x1c05a3f4, 0x1b0404cb, 0x170b3ce9, 0x1d7fffff, 0x2000ffff))
        last = rng.randrange(1 << 32)
        first = (last - rng.choice((span, span // 4, span * 4, rng.randrange(8 * span)))) % (1 << 32)
        limit = rng.choice((MAINNET_LIMIT, M.MASK))
        rows.append(f"next {bits} {last} {first} {span} {limit:064x} 0 "
                    f"{M.next_work(bits, last, first, span, limit)}")
    for x in K.base_chain()[:40]:
        rows.append(f"hash {x.hex()} {M.sha256d(x).hex()}")
    values = set()
    for hash32, bits in K.pow_rows():
        target, negative, overflow = M.set_compact(bits)
        rows.append(f"expand {bits} {target:064x} {int(negative) | 2 * int(overflow)}")
        for limit in (M.MASK, K.LOW_LIMIT, MAINNET_LIMIT):
            rows.append(f"pow {hash32.hex()} {bits} {limit:064x} {int(M.check_pow(hash32, bits, limit))}")
        values |= {target, int.from_bytes(hash32, "little")}
    rows += [f"compact {v:064x} {M.get_compact(v)}" for v in sorted(values)]
    cases = K.retarget_cases() + [("base", list(K.base_chain()[:70]), K.PARAMS, None, 0)]
    a = K.anchor_at(2)
    p = dict(K.PARAMS, bip34=5, bip66=8, bip65=11)
    b = K.Builder(p, a, seed=80)
    for k in range(10):
        b.add(version=(-1, 1, 2, 3, 4)[k % 5], time=K.T0 + 3 * K.SPACING + 40 * (k % 4))
    cases.append(("versions and times", b.headers, p, a, K.T0 + 3 * K.SPACING + 80))
    for label, headers, params, anchor, max_time in cases:
        want = M.check(headers, params, anchor, max_time)
        head, tail = model_context(params, anchor)
        rows.append(" ".join(str(v) for v in ["chain", len(headers)] + head + [max_time] + tail))
        rows += [f"{x.hex()} {s}" for x, s in zip(headers, want["status"])]
        if label == "versions and times":
            assert len(set(want["status"])) >= 4, want["status"]
    return rows


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_lane_program(golden, tmp_path, sanitize):
    """The stand-alone lane program over the fixture's rows, the compact-target sweep, every
    retarget case and chains with every status: nothing is preloaded, the program is its own
    process."""
    exe = tmp_path / "header_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-O1", "-std=c++17"] + flags +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", str(exe),
                           os.path.join(HERE, "native", "header_host.cpp")])
    rows = lane_rows(golden)
    assert len(rows) > 10000
    data = tmp_path / "rows.txt"
    data.write_text("\n".join(rows) + "\n")
    p = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and " 0 mismatches" in p.stdout, (p.returncode, p.stdout, p.stderr[-3000:])
