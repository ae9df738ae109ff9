"""CPU: the header entries' symbols are declared in include/bcc_amd.h and exported by
librbc_amd.so, the ctypes mirrors have the C sizes and offsets, null, zero and out-of-range
arguments are refused, and the product library answers on its host route with every GPU hidden."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

import bitcoinconsensus_amd as B
import engine_stub
import header_cases as K
import header_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "rust-bitcoinconsensus_amd")
SYMBOLS = ("bcc_headers_batch", "mi_pow_check_tuples", "bcc_last_header_stats", "bcc_set_header_round",
           "bcc_header_last_timing_ms")


def test_symbols_are_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bcc_amd.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
    for s in ("bcc_header_params", "bcc_header_anchor", "bcc_header_stats"):
        assert re.search(r"}\s*%s;" % s, header), s
    if not os.path.exists(B.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", PKG, "-j8"])
    lib = ctypes.CDLL(B.LIB_PATH)
    assert not [s for s in SYMBOLS if not hasattr(lib, s)]
    stub = engine_stub.load()
    assert not [s for s in SYMBOLS if not hasattr(stub, s)]


def test_python_constants_mirror_the_header():
    header = open(os.path.join(ROOT, "include", "bcc_amd.h")).read()
    found = re.findall(r"#define BCC_(HEADER_\w+) (\d+)", header)
    assert len(found) == 7
    for name, value in found:
        assert getattr(B, name) == getattr(M, name[7:]) == int(value), name


def test_python_structs_match_c_layout(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bcc_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n",'
                   ' sizeof(bcc_header_params), offsetof(bcc_header_params, pow_target_spacing),'
                   ' offsetof(bcc_header_params, bip65_height), sizeof(bcc_header_anchor),'
                   ' offsetof(bcc_header_anchor, hash), offsetof(bcc_header_anchor, bits),'
                   ' offsetof(bcc_header_anchor, n_times), offsetof(bcc_header_anchor, period_first_time),'
                   ' sizeof(bcc_header_stats), offsetof(bcc_header_stats, device_retries)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P, A, S = B.HeaderParams, B.HeaderAnchor, B.HeaderStats
    assert got == [ctypes.sizeof(P), P.pow_target_spacing.offset, P.bip65_height.offset, ctypes.sizeof(A),
                   A.hash.offset, A.bits.offset, A.n_times.offset, A.period_first_time.offset,
                   ctypes.sizeof(S), S.device_retries.offset]


def test_null_zero_and_out_of_range_arguments():
    L = K.bind(engine_stub.load())
    f = L.bcc_headers_batch
    h = K.base_chain()[0]
    p = K.c_params(K.PARAMS)
    st = (ctypes.c_int * 1)()
    work = ctypes.create_string_buffer(b"\xee" * 32, 32)
    ok = lambda params=p, anchor=None, headers=h, n=1, status=st: f(headers, n, params, anchor, 0, None, status,
                                                                   work, 0)
    assert ok() == 1 and int.from_bytes(work.raw, "little") == M.block_proof(K.LOW_BITS)
    # nothing to do: 0, and the work is zero, whatever else is null
    assert f(None, 0, None, None, 0, None, None, work, 0) == 0 and work.raw == bytes(32)
    assert f(None, 0, None, None, 0, None, None, None, 0) == 0
    assert ok(headers=None) == -1 and ok(params=None) == -1 and ok(status=None) == -1
    assert f(h, 1, p, None, 0, None, st, None, 0) == 1  # hash_out and chain_work_out are optional

    def params(**kw):
        return ctypes.byref(K.c_params(dict(K.PARAMS, **kw)))

    assert ok(params=params(spacing=0)) == -1 and ok(params=params(timespan=0)) == -1
    assert ok(params=params(spacing=-1)) == -1 and ok(params=params(timespan=-16, spacing=-1)) == -1
    assert ok(params=params(timespan=15, spacing=16)) == -1          # interval 0
    assert ok(params=params(timespan=1 << 30, spacing=1 << 26)) == -1  # 4 * timespan leaves 32 bits
    assert ok(params=params(timespan=(1 << 30) - 1, spacing=1 << 26)) == 1
    mindiff = B.HeaderParams.make(K.LOW_LIMIT, 16, 1, allow_min_difficulty=True)
    assert ok(params=ctypes.byref(mindiff)) == -1                    # the one case that is out of scope

    def anchor(**kw):
        a = dict(K.anchor_at(3), **kw)
        return ctypes.byref(K.c_anchor(a))

    good = K.Builder(K.PARAMS, K.anchor_at(3)).add().headers[0]
    assert ok(anchor=anchor(), headers=good) == 1
    assert ok(anchor=anchor(height=-1), headers=good) == -1
    assert ok(anchor=anchor(times=[]), headers=good) == -1
    twelve = K.c_anchor(K.anchor_at(3))
    twelve.n_times = 12
    assert ok(anchor=ctypes.byref(twelve), headers=good) == -1
    assert ok(anchor=anchor(height=(1 << 31) - 2), headers=good) >= 0   # height 2^31 - 1: the last one
    assert ok(anchor=anchor(height=(1 << 31) - 1), headers=good) == -1


_PRODUCT_CHILD = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import bitcoinconsensus_amd as B
import header_cases as K
import header_model as M
base = list(K.base_chain())[:100]
got = K.run(None, base, K.PARAMS)
assert got == M.check(base, K.PARAMS)
st = B.last_header_stats()
assert st == dict(headers=100, device_rounds=0, host_rounds=1, device_retries=0), st
rows = K.pow_rows()[:1500]
want = bytes(M.check_pow(h, b, K.LOW_LIMIT) for h, b in rows)
assert B.pow_check_tuples(b"".join(h for h, _ in rows), [b for _, b in rows], K.LOW_LIMIT) == want
assert B.last_header_stats()["device_rounds"] == 0
assert B.host_fallback_rounds() == 0
assert B.header_last_timing_ms() == dict(hash_kernel=0, context_kernel=0, upload=0, download=0)
print("ok")
"""


@pytest.mark.skipif(not os.path.exists(B.LIB_PATH), reason="librbc_amd.so is not built")
def test_product_library_on_its_host_route_without_a_device():
    """librbc_amd.so with the small-round threshold on and every GPU hidden from the child: batches
    below the entry's threshold are evaluated by the host and open no device."""
    env = dict(os.environ, BCC_HOST_SMALL_ROUND="16", HIP_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", _PRODUCT_CHILD, PKG, HERE], capture_output=True,
                       text=True, timeout=300, env=env)
    assert p.returncode == 0 and "ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-2000:])
