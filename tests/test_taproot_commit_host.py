"""CPU: the script-path commitment lane code and host row builder
(rust-bitcoinconsensus_amd/csrc/taproot_commit.h, compiled for the host by
tests/native/commit_host.cpp -- test-only) against every case of tests/golden/taproot_commit.json.gz
(verdicts, errors and leaf hashes recorded from the reference) and, where oracle/_ref is built,
against the live reference on a fresh random batch."""
import ctypes
import os
import random
import subprocess

import pytest

import bitcoinconsensus_amd as B
import commit_cases as C
from oracle_ctypes import Reference, reference_available

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "native", "_build", "commit_host.so")
CSRC = os.path.join(HERE, "..", "rust-bitcoinconsensus_amd", "csrc")


class HostLib:
    """The C ABI's two entry points over the host build of the lane code."""

    def __init__(self, L):
        self.L = L
        L.commit_host_batch.argtypes = [ctypes.POINTER(B.TaprootCommit), ctypes.c_size_t,
                                        ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                        ctypes.c_void_p, ctypes.c_uint]
        for f in (L.commit_tweak_check, L.commit_tweak_check_grouped):
            f.argtypes = [ctypes.c_char_p] * 5 + [ctypes.c_size_t] * (1 + (f is L.commit_tweak_check_grouped))
            f.restype = None
        self.split = 1

    def bcc_taproot_commit_batch(self, arr, n, ret, err, hs, device):
        return self.L.commit_host_batch(arr, n, ret, err, hs, self.split)

    def tweak_check(self, ts, group=None):
        q, par, p, t = C.tuple_rows(ts)
        out = ctypes.create_string_buffer(max(1, len(ts)))
        if group is None:
            self.L.commit_tweak_check(q, par, p, t, out, len(ts))
        else:
            self.L.commit_tweak_check_grouped(q, par, p, t, out, len(ts), group)
        return list(out.raw[: len(ts)])


@pytest.fixture(scope="module")
def host():
    src = os.path.join(HERE, "native", "commit_host.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        tmp = SO + f".{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-I" + os.path.join(HERE, "..", "include"), "-o", tmp, src])
        os.replace(tmp, SO)
    return HostLib(ctypes.CDLL(SO))


@pytest.fixture(scope="module")
def golden():
    return C.load_golden()


def check_spends(out, leaves, cases):
    """Verdict, error and leaf hash of every case: none left out."""
    assert len(out) == len(cases) == len(leaves)
    bad = [(c["cls"], out[i], (c["ret"], c["serror"])) for i, c in enumerate(cases)
           if out[i] != (c["ret"], c["serror"])]
    assert not bad, bad[:10]
    bad = [c["cls"] for i, c in enumerate(cases) if leaves[i] != (c["leaf"] or bytes(32))]
    assert not bad, bad[:10]


def test_golden_file_covers_the_cases_asked_for(golden):
    """The committed file holds what its generator promises (a stale or cut file fails here)."""
    spends, tuples = golden
    valid = [c for c in spends if c["ret"] == 1]
    depths = {(len(c["control"]) - 33) // 32 for c in valid}
    assert {0, 1, 2, 7, 127, 128} <= depths
    lengths = {len(c["script"]) for c in valid}
    assert {0, 1, 53, 54, 61, 62, 63, 117, 118, 252, 253, 65535, 65536} <= lengths
    assert any(69000 < n < 71000 for n in lengths)
    assert {c["control"][0] & 1 for c in valid} == {0, 1}
    assert {0xC0, 0xC2, 0xFE} <= {c["control"][0] & 0xFE for c in valid}
    assert all(c["script"] == b"\x51" for c in valid if c["control"][0] & 0xFE == 0xC0)
    for what in ("parity", "p", "node", "script", "q"):
        assert any(c["cls"].endswith("flip_" + what) and c["serror"] == 39 for c in spends), what
    assert {32, 34, 64, 33 + 32 * 129} <= {len(c["control"]) for c in spends if c["serror"] == 47}
    by = {t["cls"]: t["verdict"] for t in tuples}
    want = dict(valid=1, wrong_parity=0, t_zero_par0=1, t_zero_par1=0, t_eq_n=0, t_max=0,
                t_n_minus_1=1, doubling=1, infinity_q0=0, infinity_qp=0, p_off_curve=0,
                p_eq_prime=0, p_eq_prime_plus_1=0, parity_2=0, q_plus_1=0)
    assert {k: by.get(k) for k in want} == want
    assert any(k.startswith("mix_") for k in by)


def test_commit_lane_code_matches_every_golden_spend(host, golden):
    spends, _ = golden
    for host.split in (1, 7):
        out, leaves = B.taproot_commit_batch(spends, tapleaf=True, library=host)
        check_spends(out, leaves, spends)
    host.split = 1


def test_commit_one_item_per_call_equals_the_batch(host, golden):
    """The row builder's offsets: each item alone gives what it gives inside the batch."""
    spends, _ = golden
    small = [c for c in spends if len(c["script"]) < 300]
    for c in small:
        out, leaves = B.taproot_commit_batch([c], tapleaf=True, library=host)
        check_spends(out, leaves, [c])


def test_tweak_lane_code_matches_every_golden_tuple(host, golden):
    _, tuples = golden
    ts = [(t["cls"], t["q"], t["parity"], t["p"], t["t"]) for t in tuples]
    want = [t["verdict"] for t in tuples]
    got = host.tweak_check(ts)
    assert [(t[0], g) for t, g, w in zip(ts, got, want) if g != w] == []
    # the kernels' grouped inversion: a decided row must not poison its group
    for group in (2, 3, 16, len(ts)):
        got = host.tweak_check(ts, group)
        assert [(group, t[0], g) for t, g, w in zip(ts, got, want) if g != w] == []


def test_leaf_message_padding_edges(host):
    """The padded leaf message against hashlib for every script length around a block edge (the
    leaf hash needs no curve: this runs everywhere)."""
    rng = random.Random(11)
    items = []
    for n in list(range(0, 200)) + [250, 251, 252, 253, 254, 255, 256, 300, 1000, 65535, 65536]:
        lv = rng.choice([0xC0, 0xC2, 0xFE, 0x02])
        script = rng.randbytes(n)
        items.append(dict(control=bytes([lv | rng.randrange(2)]) + rng.randbytes(32 + 32 * rng.randrange(3)),
                          script=script, program=rng.randbytes(32), want=C.tapleaf(lv, script)))
    out, leaves = B.taproot_commit_batch(items, tapleaf=True, library=host)
    assert [len(i["script"]) for i, h in zip(items, leaves) if h != i["want"]] == []
    assert all(o == (0, 39) for o in out)  # random programs commit to nothing


def test_python_struct_matches_c_layout(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bcc_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(bcc_taproot_commit),'
                   ' offsetof(bcc_taproot_commit, script_len), offsetof(bcc_taproot_commit, program32));'
                   ' return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(HERE, "..", "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(B.TaprootCommit), B.TaprootCommit.script_len.offset,
                   B.TaprootCommit.program32.offset]
    assert (B.SCRIPT_ERR_WITNESS_PROGRAM_MISMATCH, B.SCRIPT_ERR_TAPROOT_WRONG_CONTROL_SIZE) == (39, 47)


def test_product_library_host_rounds_match_golden():
    """The product library's own host half with every batch at or below the small-round threshold
    (no GPU needed): both entry points against every golden case, and bad arguments."""
    import sys
    code = f"""
import sys
sys.path[:0] = [{os.path.join(HERE, '..', 'rust-bitcoinconsensus_amd')!r}, {HERE!r}]
import bitcoinconsensus_amd as B
import commit_cases as C
from test_taproot_commit_host import check_spends
B.set_host_small_round(1 << 30)
spends, tuples = C.load_golden()
out, leaves = B.taproot_commit_batch(spends, tapleaf=True)
check_spends(out, leaves, spends)
assert B.taproot_commit_batch(spends, device=-1) == out
rows = [(t["cls"], t["q"], t["parity"], t["p"], t["t"]) for t in tuples]
got = B.xonly_tweak_check_tuples(*C.tuple_rows(rows))
assert list(got) == [t["verdict"] for t in tuples]
assert B.taproot_commit_batch([]) == [] and B.xonly_tweak_check_tuples(b"", b"", b"", b"") == b""
arr = (B.TaprootCommit * 1)(B.TaprootCommit(None, 33, b"", 0, bytes(32)))
import ctypes
r, e = (ctypes.c_int * 1)(7), (ctypes.c_int * 1)(7)
assert B.lib().bcc_taproot_commit_batch(arr, 1, r, e, None, 0) == -1 and (r[0], e[0]) == (7, 7)
print("ok")
"""
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-2000:])


@pytest.mark.skipif(not reference_available(), reason="oracle/_ref not built")
def test_commit_lane_code_vs_live_reference(host):
    R = Reference()
    T = C.RefTweak(R)
    rng = random.Random(0xC0111)
    items = []
    for _ in range(300):
        lv = rng.choice([0xC0, 0xC2, 0xC4, 0xFE, 0x0A])
        script = b"\x51" if lv == 0xC0 else rng.randbytes(rng.choice([0, 1, 30, 54, 55, 62, 64, 119, 300]))
        it = C.make_spend(rng, rng.choice([0, 1, 2, 3, 5, 11, 40]), script, lv)
        if rng.random() < 0.4:
            it = C.mutate(rng, it, rng.choice(C.applicable_mutations(it)))
        elif rng.random() < 0.1:
            it = dict(it, control=it["control"][: rng.randrange(len(it["control"]))])
        items.append(it)
    out = B.taproot_commit_batch(items, library=host)
    bad = [(i, out[i], C.ref_spend(R, it)) for i, it in enumerate(items) if out[i] != C.ref_spend(R, it)]
    assert not bad, bad[:10]
    assert sum(o[0] for o in out) > 100
    ts = C.edge_tuples(rng) + C.random_tuples(rng, 300)
    got = host.tweak_check(ts, 16)
    bad = [(t[0], g) for t, g in zip(ts, got) if g != T.check(*t[1:])]
    assert not bad, bad[:10]


def test_tweak_lane_code_structured_scalars(host):
    """The comb's scalar families as tweaks (tests/golden/structured_scalars.npz: powers of two and
    their neighbours, every window at the table's extremes, zero), rows and invalid twins, one
    inversion per row and grouped."""
    from fixtures import structured_scalars
    rows = structured_scalars()["tweak"]
    ts = [(t["cls"], t["q"], t["parity"], t["p"], t["t"]) for t in rows]
    want = [t["verdict"] for t in rows]
    assert sum(want) >= 2000 and want.count(0) >= 2000
    for group in (None, 16):
        got = host.tweak_check(ts, group)
        assert [(group, t[0], g) for t, g, w in zip(ts, got, want) if g != w] == []
