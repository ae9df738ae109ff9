"""Shared cases of the device paths for the remaining ECDSA-era hash types (bcc_set_device_hashtypes):
legacy NONE / SINGLE / ANYONECANPAY checks (pipeline.h LinJob, sighash.hip legacy_in_kernel) and
BIP143 SIGHASH_SINGLE checks (WinJob, bip143_in_kernel).  Transactions of random bytes from
sighash_model.rand_tx, expected digests from sighash_model.sighash (test_sighash_geometry.py pins
that model to the reference).  Every check carries a geometry record computed from the shapes alone,
never from a digest; test_hashtype_host.py asserts what the records cover.

Also the loader of the native test library (tests/native/hashtype_host.cpp) that runs the
product's job builder and host evaluation without a device."""
import ctypes
import functools
import os
import random
import subprocess

import sighash_model as M
from sighash_model import cs_len

SEED = 0x4A5B17

# (hash type, name of its base x ANYONECANPAY class).  The 32-bit values with garbage in the bits
# SignatureHash ignores (bits 5-6 and 8-31) sit over the same five classes; the negative one is
# 0x80000003 as the int32 a script's hash type byte never gives but the interface admits.
BASE_TYPES = [(2, "none"), (3, "single"), (0x81, "all_acp"), (0x82, "none_acp"), (0x83, "single_acp")]
GARBAGE_TYPES = [(0x7fffff02, "none"), (0x80000003 - (1 << 32), "single"),
                 (0x5a5a5ac2, "none_acp"), (0xabcdefe3 - (1 << 32), "single_acp"),
                 (0x00100081, "all_acp"), (0x80, "all_acp"), (0x84, "all_acp")]
CLASSES = dict(BASE_TYPES + GARBAGE_TYPES)
RESIDUES = (55, 56, 63, 0)  # preimage length mod 64 at the padding edges of xs_final_d


def code_with_separators(rng, n, seps):
    """n single-byte opcodes, `seps` of them OP_CODESEPARATOR (n >= seps)."""
    code = bytearray(M.op_script(rng, n))
    for i in rng.sample(range(n), seps):
        code[i] = M.OP_CODESEPARATOR
    return bytes(code)


def legacy_geometry(nin, out_lens, sig_lens, witness, k, code_len, seps, ht):
    """Lengths of the preimage CTransactionSignatureSerializer writes, from the shapes alone."""
    base, acp = ht & 0x1f, bool(ht & 0x80)
    field = code_len - seps
    cl = cs_len(field) + field
    bug = base == 3 and k >= len(out_lens)
    nins = 1 if acp else nin
    n = 4 + cs_len(nins) + 41 * (nins - 1) + 36 + cl + 4
    if base == 2:
        n += 1
    elif base == 3:
        n += cs_len(k + 1) + 9 * k + M.outs_len(out_lens[k:k + 1])
    else:
        n += cs_len(len(out_lens)) + M.outs_len(out_lens)
    n += 8
    return dict(kind="legacy_rawtx", cls=CLASSES[ht], ht=ht & 0xffffffff, nin=nin, k=k,
                nout=len(out_lens), out_lens=tuple(out_lens[:4]), sig_lens=tuple(sig_lens[:4]),
                witness=witness, stripped=witness and len(out_lens) > 0, code_len=code_len,
                seps=seps, cl=cl, single_bug=bug, pre_len=None if bug else n,
                in_count_cs=cs_len(nins), single_count_cs=cs_len(k + 1) if base == 3 else None)


def legacy_sweep(seed=SEED + 1):
    rng = random.Random(seed)
    checks, geoms = [], []

    def add(tx, nin, outs, sigs, witness, k, code_len, seps, ht):
        checks.append((tx, code_with_separators(rng, code_len, seps), k, ht, 0, 0))
        geoms.append(legacy_geometry(nin, outs, sigs, witness, k, code_len, seps, ht))

    out_cycle, sig_cycle = (0, 25, 252, 253), (0, 5, 107, 253)
    j = 0
    # input and output counts: 253 / 254 inputs cross the three-byte input count, SINGLE at the
    # last input of 253 the three-byte count of nin + 1 outputs; outputs 0, 1, nin, nin + 1 and
    # more put the SINGLE bug beside the last valid index
    for nin in (1, 2, 3, 5, 252, 253, 254):
        big = nin >= 252
        types = BASE_TYPES + (GARBAGE_TYPES[:2] if big else GARBAGE_TYPES)
        for nout in sorted({0, 1, nin, nin + 1, nin + 3}):
            witness = j % 2 == 1
            # (the many outputs of the large transactions stay short but for the first few)
            outs = tuple(out_cycle[(i + j) % 4] if not big or i < 4 or i >= nout - 2 else (i % 3) * 11
                         for i in range(nout))
            sigs = [sig_cycle[(i + j) % 4] if not big or i < 8 else (0, 5, 72)[i % 3]
                    for i in range(nin)]
            tx = M.rand_tx(rng, nin, outs, sigs, witness)
            for k in sorted({0, nin // 2, nin - 1}):
                for ht, _ in types:
                    add(tx, nin, outs, sigs, witness, k, (25, 0, 35, 71, 107)[j % 5], 0, ht)
            j += 1
    # code lengths 0-70 and 252-254, with and without OP_CODESEPARATORs, for every class: 71
    # consecutive lengths walk the preimage length through every residue mod 64
    for witness in (False, True):
        outs, sigs = (25, 0, 253), [5, 0, 107]
        tx = M.rand_tx(rng, 3, outs, sigs, witness)
        for ht, _ in BASE_TYPES:
            for n in list(range(0, 71)) + [252, 253, 254]:
                k = 1  # (fixed: SINGLE's output section depends on it)
                add(tx, 3, outs, sigs, witness, k, n, 0, ht)
                if n in (0, 25, 70, 253):
                    add(tx, 3, outs, sigs, witness, 0, n, 0, ht)
                    add(tx, 3, outs, sigs, witness, 2, n, 0, ht)
                if n >= 2 and (n % 4 == 1 or n >= 252):
                    add(tx, 3, outs, sigs, witness, k, n, 1 + n % 2, ht)
    # a witness-format transaction without outputs goes up with its marker and flag
    tx = M.rand_tx(rng, 3, (), [0, 107, 5], True)
    for ht, _ in BASE_TYPES + GARBAGE_TYPES:
        for k in range(3):
            add(tx, 3, (), [0, 107, 5], True, k, 25, 0, ht)
    return checks, geoms


def bip143_single_sweep(seed=SEED + 2):
    rng = random.Random(seed)
    checks, geoms = M.bip143_single_sweep()
    checks, geoms = list(checks), [dict(g, out_len=None) for g in geoms]

    def add(tx, nin, outs, witness, k, code_len, ht):
        cl = code_len + cs_len(code_len)
        checks.append((tx, M.op_script(rng, code_len), k, ht, M._amount(rng), 1))
        has = k < len(outs)
        geoms.append(dict(kind="bip143_single", nin=nin, nout=len(outs), k=k, ht=ht,
                          code_len=code_len, cl=cl, pre_len=156 + cl, slot=156 + cl - 40,
                          has_output=has, witness=witness,
                          out_len=M.outs_len(outs[k:k + 1]) if has else None))

    # output n_in at the padding edges of the inner hash (8 + compactsize + script = 55, 56, 64
    # bytes) and across the three-byte script length; n_in >= outputs; both wire forms
    for L in (0, 55 - 9, 56 - 9, 64 - 9, 252, 253):
        for witness in (False, True):
            for outs in ((L, 25), (25, L), (L,)):
                tx = M.rand_tx(rng, 3, outs, [0, 5, 107], witness)
                for k in range(3):
                    for ht in (3, 0x83):
                        add(tx, 3, outs, witness, k, (25, 0, 253)[k], ht)
    for witness in (False, True):  # no outputs at all (the witness form keeps marker and flag)
        tx = M.rand_tx(rng, 2, (), [0, 72], witness)
        for k in range(2):
            for ht in (3, 0x83):
                add(tx, 2, (), witness, k, 25, ht)
    return checks, geoms


SWEEPS = {"legacy_rawtx": legacy_sweep, "bip143_single_rawtx": bip143_single_sweep}


@functools.lru_cache(maxsize=None)
def sweep(name):
    """(checks, geometry records, the model's digests) of one sweep; built once."""
    checks, geoms = SWEEPS[name]()
    assert len(checks) == len(geoms)
    return checks, geoms, [M.sighash(*c) for c in checks]


@functools.lru_cache(maxsize=None)
def golden_checks(name):
    """The committed goldens as checks: 'legacy' = the 500 sighash_legacy.json rows (the reference's
    own vectors), 'random' = the 1,200 sighash_random.json.gz checks; (checks, expected)."""
    import test_sighash_goldens as G
    checks, exp = G.legacy_checks() if name == "legacy" else G.random_checks()
    return checks, [bytes.fromhex(e) for e in exp]


def legacy_non_all(checks):
    """The legacy checks add_sighash_job does not send to the template path."""
    return [c for c in checks if c[5] == 0 and not M.legacy_all_type(c[3])]


def mismatches(name, got, exp, geoms=None, limit=8):
    assert len(got) == len(exp), (name, len(got), len(exp))
    bad = [i for i in range(len(exp)) if bytes(got[i]) != exp[i]]
    if not bad:
        return ""
    lines = [f"{name}: {len(bad)} of {len(exp)} digests differ"]
    lines += [f"  [{i}] {geoms[i] if geoms else ''}" for i in bad[:limit]]
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------
# tests/native/hashtype_host.cpp: build_sighash_checks + host_sighash of the engine's host code

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KIND_FIELDS = ("legacy_template", "legacy_rawtx", "bip143_rawtx", "bip143_rawtx_single",
               "host_preimage", "single_bug", "host_hashed")


class Kinds(ctypes.Structure):
    _fields_ = [(f, ctypes.c_size_t) for f in KIND_FIELDS]


@functools.lru_cache(maxsize=None)
def host_lib():
    """(engine_host.so, hashtype_host.so): the second links the first, so both share one engine."""
    import engine_stub
    E = engine_stub.load()
    src = os.path.join(HERE, "native", "hashtype_host.cpp")
    so = os.path.join(HERE, "native", "_build", "hashtype_host.so")
    deps = [src, engine_stub.SO]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC",
                               "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "rust-bitcoinconsensus_amd", "csrc"),
                               "-o", tmp, src, engine_stub.SO, "-Wl,-rpath," + os.path.dirname(so)])
        os.replace(tmp, so)
    H = ctypes.CDLL(so)
    E.bcc_set_device_hashtypes.argtypes = [ctypes.c_int]
    E.bcc_last_sighash_kinds.argtypes = [ctypes.POINTER(Kinds)]
    E.bcc_last_sighash_kinds.restype = None
    return E, H


def host_sighash(checks, on):
    """The checks through build_sighash_checks and host_sighash with the switch set to `on`:
    (digests, kinds dict, job bytes).  Leaves the switch off."""
    import bitcoinconsensus_amd as B
    E, H = host_lib()
    n = len(checks)
    arr = (B.SighashCheck * n)()
    keep = []
    for i, (tx, code, nin, ht, amount, sv) in enumerate(checks):
        tb = ctypes.create_string_buffer(bytes(tx), max(1, len(tx)))
        cb = ctypes.create_string_buffer(bytes(code), max(1, len(code)))
        keep += [tb, cb]
        ht = int(ht) & 0xffffffff
        arr[i] = B.SighashCheck(ctypes.addressof(tb), len(tx), ctypes.addressof(cb), len(code), nin,
                                ht - (1 << 32) if ht >= 1 << 31 else ht, amount, sv)
    out = ctypes.create_string_buffer(32 * max(1, n))
    kinds, nbytes = Kinds(), ctypes.c_size_t(0)
    E.bcc_set_device_hashtypes(1 if on else 0)
    try:
        rc = H.hashtype_host_sighash(arr, ctypes.c_size_t(n), out, ctypes.byref(kinds),
                                     ctypes.byref(nbytes))
    finally:
        E.bcc_set_device_hashtypes(0)
    assert rc == 0, rc
    return ([out.raw[32 * i:32 * i + 32] for i in range(n)],
            {f: getattr(kinds, f) for f in KIND_FIELDS}, nbytes.value)
