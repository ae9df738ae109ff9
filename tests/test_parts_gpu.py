"""GPU: device rounds staged from several host parts (one per host shard), where the parts differ
in the job kinds they hold.  A part's records are rebased into the round's concatenation by the
rule of csrc/pipeline.h (PartBase / TapBase, rebase: device_batch.hip DeviceBatch::stage_parts,
taproot_round.hip through taproot_fill_part); a part that lacks a kind contributes a zero-length
segment to that kind's arrays, the shape at which a wrong base shows.  test_rebase_rule.py checks
the same rule on the host.

The batches are larger than a few dozen items because the host pass only cuts shards from 64
verify_batch items (engine.cpp chunk_start) or 2,048 Taproot checks (taproot.cpp build_round) per
worker: below that a round has one part and nothing is rebased.  Every Taproot message is
device-built: the product has no caller of the host-built TaprootJobs arrays (add_msg), which
test_rebase_rule.py fills by hand instead."""
import os

import pytest

import bitcoinconsensus_amd as B
import mixed_input_cases as MC
from fixtures import taproot_checks
from test_hashtype_host import spends
from test_taproot_host import check_against_golden

pytestmark = pytest.mark.gpu
SMALL_ROUND = int(os.environ.get("BCC_HOST_SMALL_ROUND", "16"))  # (conftest.py sets the suite's)


def spent_outputs(blob):
    """[(amount, script)] of a serialized std::vector<CTxOut> with fewer than 253 short outputs."""
    n, o, out = blob[0], 1, []
    assert n < 253
    for _ in range(n):
        amount, ln = int.from_bytes(blob[o:o + 8], "little"), blob[o + 8]
        assert ln < 253
        out.append((amount, blob[o + 9:o + 9 + ln]))
        o += 9 + ln
    assert o == len(blob)
    return out


def ecdsa_items():
    """(kind, (spk, amount, tx, nin), expected ret) of the signed hash-type fixture and of the
    mixed transactions' pre-Taproot inputs, with the reference's answers at flags 0xE15."""
    items, flags, tuples = spends()
    assert flags == MC.ALL
    out = [(it["kind"], t, it["ret"]) for it, t in zip(items, tuples)]
    for t in MC.mixed_txs():
        outs = spent_outputs(t["spent"])
        for k, i in enumerate(t["inputs"]):
            if i["kind"] in MC.ECDSA_KINDS:
                out.append((i["kind"], (outs[k][1], outs[k][0], t["tx"], k), i["ret"]))
    return out


def test_verify_batch_shards_of_different_job_kinds():
    """Three host shards: the first holds only P2WPKH items (BIP143 jobs and key-hash records: no
    template job, no legacy raw-tx job), the last only legacy P2PKH / P2SH ones (no BIP143 job, no
    raw tx of one, no key-hash record of a witness program), the middle one everything."""
    every = ecdsa_items()
    cycle = lambda xs, n: [xs[i % len(xs)] for i in range(n)]  # noqa: E731
    wpkh = [e for e in every if e[0] == "p2wpkh"]
    legacy = [e for e in every if e[0] in ("p2pkh", "p2sh_multisig", "p2sh_2of3")]
    rest = [e for e in every if e[0] not in ("p2wpkh", "p2pkh")]
    assert len(wpkh) >= 64 and len(legacy) >= 64 and len(rest) >= 64
    batch = cycle(wpkh, 120) + rest[::2] + cycle(legacy, 120)
    # the shards are cut at the first transaction starting at or after 1/3 and 2/3 of the items
    # (engine.cpp shard_bounds): inside the P2WPKH run and inside the legacy run
    n = len(batch)
    assert n >= 256 and n // 3 + 8 <= 120 and 2 * n // 3 >= n - 120
    tuples, exp = [b[1] for b in batch], [b[2] for b in batch]

    def run(threads):
        B.set_host_threads(threads)
        rc, res = B.verify_batch_raw(tuples, MC.ALL)
        return rc, res, B.last_sighash_kinds(), B.last_batch_stats()

    fallbacks = B.host_fallback_rounds()
    B.set_host_small_round(0)
    B.set_device_hashtypes(True)
    B.set_device_key_hash(True)
    try:
        rc3, res3, k3, s3 = run(3)
        rc1, res1, k1, s1 = run(1)
    finally:
        B.set_host_threads(0)
        B.set_device_key_hash(True)
        B.set_device_hashtypes(False)
        B.set_host_small_round(SMALL_ROUND)
    bad = [(i, batch[i][0], res3[i], exp[i]) for i in range(n) if res3[i][0] != exp[i]]
    assert not bad, bad[:10]
    assert rc3 == sum(exp) and 0 < rc3 < n
    assert res3 == res1 and rc3 == rc1
    # every round ran on the device, as device jobs of every kind
    assert B.host_fallback_rounds() == fallbacks
    for k, s in ((k3, s3), (k1, s1)):
        assert s["host_rounds"] == 0 and s["rounds"] >= 1 and s["host_hashed"] == 0, s
        assert s["device_key_hashes"] > 0, s
        assert min(k["legacy_template"], k["legacy_rawtx"], k["bip143_rawtx"],
                   k["bip143_rawtx_single"]) > 0 and k["host_preimage"] == 0, k
    assert k3 == k1


def test_taproot_parts_of_different_check_kinds():
    """Three host parts of 2,155 checks each: the first holds only key path checks without annex
    under SIGHASH_DEFAULT / ALL (no byte in the ext blob), the last only tapscript ones (every job
    with ext bytes), the middle one every committed case."""
    cases = taproot_checks()
    n = len(cases)
    assert n >= 2048
    cycle = lambda xs: [xs[i % len(xs)] for i in range(n)]  # noqa: E731
    plain = [c for c in cases if c["sigversion"] == 0 and c["annex"] is None and c["ret"] == 1
             and (len(c["sig"]) == 64 or c["sig"][64] == 1)]
    script = [c for c in cases if c["sigversion"] == 1 and c["ret"] in (0, 1) and c["sighash"] is not None]
    assert len(plain) >= 8 and len(script) >= 64
    batch = cycle(plain) + cases + cycle(script)

    def run(threads):
        B.set_host_threads(threads)
        out, hs = B.taproot_verify_batch(batch, sighashes=True)
        return out, hs, B.last_taproot_stats()

    B.set_host_small_round(0)
    try:
        out3, hs3, s3 = run(3)
        out1, hs1, s1 = run(1)
    finally:
        B.set_host_threads(0)
        B.set_host_small_round(SMALL_ROUND)
    check_against_golden(out3, hs3, batch)
    assert out3 == out1 and hs3 == hs1
    for s in (s3, s1):
        assert s["checks"] > 2 * n and s["rounds"] >= 1, s
        assert s["host_rounds"] == 0 and s["host_checks"] == 0 and s["device_retries"] == 0, s
