"""bench.py's plain run and --dump-outputs.

CPU: dump_outputs writes float32 .npy files, keeps small arrays whole and cuts a large one to the
same seeded sample of rows on every call, under the size bound.
GPU: a plain run prints only the headline line (nothing of a --full run) and its dump is the last
step's verdicts and sighashes, equal to what the staged workload itself reports for those inputs.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 400_000)  # share: 200,000 - 4,096 bytes per array
    rng = np.random.default_rng(1)
    small = rng.integers(0, 2, 1000, dtype=np.uint8)
    big = rng.integers(0, 256, (5000, 32), dtype=np.uint8)   # 640,000 bytes as float32
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"verdicts": small, "sighashes": big})
    va, sa = np.load(tmp_path / "a" / "verdicts.npy"), np.load(tmp_path / "a" / "sighashes.npy")
    sb = np.load(tmp_path / "b" / "sighashes.npy")
    assert va.dtype == np.float32 and sa.dtype == np.float32
    assert np.array_equal(va, small)
    rows = (200_000 - 4096) // 128
    assert sa.shape == (rows, 32) and np.array_equal(sa, sb)
    # the sample: distinct rows of the array, in their original order
    keep = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(5000, rows, replace=False))
    assert len(set(keep)) == rows and np.array_equal(sa, big[keep])
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 400_000


@pytest.mark.gpu
def test_plain_run_prints_headline_and_dumps_last_step(tmp_path):
    n, seed = 20_000, 0x5EED0001
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n", str(n),
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "d")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "verifies/s"
    assert d["higher_is_better"] is True and d["dtype"] == "u32" and d["ms_per_step"] > 0
    assert abs(d["value"] - n / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    for k in ("roofline", "cpu_baseline", "sustained", "drop_in_end_to_end", "c3_block_replay"):
        assert k not in d
    v, m = np.load(tmp_path / "d" / "verdicts.npy"), np.load(tmp_path / "d" / "sighashes.npy")
    assert v.dtype == np.float32 and m.dtype == np.float32
    import bitcoinconsensus_amd as B
    wl = B.Workload(n, seed=seed, device=0)
    wl.run()
    assert np.array_equal(v, np.frombuffer(wl.verdicts(), np.uint8))
    assert np.array_equal(m, np.frombuffer(wl.msgs(), np.uint8).reshape(-1, 32))
    assert v.shape == (n,) and v.all()
