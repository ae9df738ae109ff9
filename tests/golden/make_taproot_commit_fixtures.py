"""Generate tests/golden/taproot_commit.json.gz (run where the reference build oracle/_ref exists).

    python3 tests/golden/make_taproot_commit_fixtures.py

BIP341 script-path commitment checks: VerifyWitnessProgram's control-size rule and
VerifyTaprootCommitment (depend/bitcoin/src/script/interpreter.cpp:1909-1914, 1834-1853) and, one
layer below, secp256k1_xonly_pubkey_parse + secp256k1_xonly_pubkey_tweak_add_check.  The spends and
tuples are BUILT with plain Python integer curve arithmetic (tests/commit_cases.py); every recorded
verdict and error comes from the REFERENCE, by two routes: whole spends through VerifyScript
(Reference.capture_script with P2SH | WITNESS | TAPROOT on a one-input tx whose witness is
[script, control]; a leaf version other than 0xc0 succeeds as soon as the commitment holds, 0xc0
runs the script, so its script is OP_1), tuples through the secp256k1 functions the reference
build exports.  The recorded TapLeaf hash of a spend is pinned by the reference as well: the
program q is built from it, so the reference returning 1 for the spend (or, for a case that is
itself invalid, for a valid spend built around the same leaf version and script) means it
recomputed the same hash.  Scripts of 1000 bytes or more are stored as (seed, length).

Cases: depths 0, 1, 2, 7, 127, 128; script lengths 0, 1, 53, 54, 61, 62, 63, 117, 118, 252, 253,
65535, 65536, 70001 (the 55/56-byte padding edge, the block edges and the compact-size steps of
the leaf message); leaf versions 0xc0 (script OP_1), 0xc2, 0xc4, 0xfe and others (never 0x50: the
reference would take such a control block for the annex); both parities; nodes above, below and equal to the running hash; every one-bit mutation (parity,
p, a node, the script, q); control sizes 32, 34, 33 + 31, 33 + 32 * 129, 0; tuple edge rows
(t = 0, t >= n, t = n - 1, doubling, infinity, p off the curve / not below the prime, q off by
one or not canonical, parity bytes above 1) alone and interleaved with valid rows.
"""
import gzip
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import commit_cases as C  # noqa: E402
from oracle_ctypes import Reference  # noqa: E402

LONG = 1000


def main():
    R = Reference()
    T = C.RefTweak(R)
    rng = random.Random(0x7A9C0117)
    spends = []
    seeds = iter(range(1, 1 << 20))

    def script_of(length, leaf_version):
        """(script, how it is stored)"""
        if leaf_version == 0xC0:
            assert length == 1
            return b"\x51", None
        if length >= LONG:
            s = next(seeds)
            return C.seeded_script(s, length), [s, length]
        return rng.randbytes(length), None

    def pin_leaf(leaf_version, script):
        """The reference recomputes this leaf hash: a valid depth-0 spend around it passes."""
        if leaf_version == 0xC0 and script != b"\x51":
            return  # the script would run; its leaf hash is pinned through 0xc2's code path only
        it = C.make_spend(rng, 0, script, leaf_version)
        assert C.ref_spend(R, it) == (1, 0), ("pin", leaf_version, len(script))

    def record(cls, it, stored=None, flips=None, control_seed=None, pinned=False):
        ret, serr = C.expected_commit(*C.ref_spend(R, it))
        size_ok = serr != C.ERR_CONTROL_SIZE
        c = dict(cls=cls, program=it["program"].hex(), ret=ret, serror=serr, leaf=None)
        if size_ok:
            lv = it["control"][0] & 0xFE
            if ret != 1 and not pinned:
                pin_leaf(lv, it["script"])
            c["leaf"] = C.tapleaf(lv, it["script"]).hex()
        if control_seed:
            c["control_seed"] = control_seed
        else:
            c["control"] = it["control"].hex()
        if stored:
            c["script_seed"] = stored
            if flips:
                c["script_flip"] = flips
        else:
            c["script"] = it["script"].hex()
        spends.append(c)
        return ret, serr

    def family(cls, depth, length, leaf_version, nodes=None, mutations=True, want_valid=True):
        script, stored = script_of(length, leaf_version)
        it = C.make_spend(rng, depth, script, leaf_version, nodes)
        got = record(cls, it, stored)
        if want_valid:
            assert got == (1, 0), (cls, got)
        if not mutations:
            return it
        for what in C.applicable_mutations(it):
            m = C.mutate(rng, it, what)
            flips = None
            if what == "script" and stored:
                (off, bit), = [(i, a ^ b) for i, (a, b) in enumerate(zip(script, m["script"])) if a != b]
                flips = [[off, bit]]
            got = record(f"{cls}/flip_{what}", m, stored, flips, pinned=what != "script")
            assert got == (0, C.ERR_MISMATCH), (cls, what, got)
        return it

    versions = [0xC2, 0xC4, 0xFE, 0xC6, 0x66, 0x7E, 0x00, 0xBE]
    # depths x a few lengths
    for depth in (0, 1, 2, 7, 127, 128):
        for length, lv in ((0, 0xC2), (1, 0xC0), (33, rng.choice(versions))):
            family(f"d{depth}_l{length}_v{lv:02x}", depth, length, lv)
    # every length edge of the leaf message, at two depths
    for length in (0, 1, 53, 54, 61, 62, 63, 117, 118, 252, 253, 65535, 65536, 70001):
        for depth in (0, 3):
            lv = versions[(length + depth) % len(versions)]
            family(f"len{length}_d{depth}_v{lv:02x}", depth, length, lv, mutations=length < LONG or depth == 3)
    # both parities of the tweaked key: draw until each has been seen with each leaf-version class
    seen = set()
    while len(seen) < 4:
        lv = rng.choice([0xC0, 0xFE])
        it = C.make_spend(rng, 2, b"\x51" if lv == 0xC0 else rng.randbytes(40), lv)
        key = (lv, it["control"][0] & 1)
        if key not in seen:
            seen.add(key)
            assert record(f"parity{key[1]}_v{lv:02x}", it) == (1, 0)
    # the TapBranch order: nodes above / below / equal to the running hash, and mixes
    above = lambda k: C.b32(min(2**256 - 1, int.from_bytes(k, "big") + 1))  # noqa: E731
    below = lambda k: C.b32(max(0, int.from_bytes(k, "big") - 1))  # noqa: E731
    far_above = lambda k: bytes([min(255, k[0] + 1)]) + k[1:] if k[0] < 255 else b"\xff" * 32  # noqa: E731
    far_below = lambda k: bytes([k[0] - 1]) + k[1:] if k[0] else bytes(32)  # noqa: E731
    last_byte = lambda k: k[:31] + bytes([k[31] ^ 1])  # noqa: E731
    equal = lambda k: k  # noqa: E731
    for name, nodes in (("above", [above]), ("below", [below]), ("far_above", [far_above]),
                        ("far_below", [far_below]), ("last_byte", [last_byte]),
                        ("mixed", [above, below, far_below, far_above, last_byte, below, above])):
        family(f"order_{name}", len(nodes), 20, 0xC2, nodes)
    # an equal node: whatever the reference says (lexicographical_compare puts the node first)
    family("order_equal", 1, 20, 0xC2, [equal], want_valid=False)
    family("order_equal_mid", 3, 20, 0xC4, [above, equal, below], want_valid=False)
    # control sizes
    base0 = family("size_base_33", 0, 10, 0xC2, mutations=False)
    base = family("size_base_65", 1, 10, 0xC2, mutations=False)
    for cls, control in (("size_32", base0["control"][:32]), ("size_34", base0["control"] + b"\x00"),
                         ("size_33_31", base["control"][:64]), ("size_0", b""), ("size_1", b"\xc2"),
                         ("size_66", base["control"] + b"\x00")):
        got = record(cls, dict(base, control=control))
        assert got == (0, C.ERR_CONTROL_SIZE), (cls, got)
    s = next(seeds)
    for cls, n in (("size_129_nodes", 33 + 32 * 129), ("size_129_nodes_plus_1", 33 + 32 * 129 + 1),
                   ("size_128_nodes_plus_31", 33 + 32 * 128 + 31)):
        control = C.seeded_script(s, n)
        got = record(cls, dict(base, control=control), control_seed=[s, n])
        assert got == (0, C.ERR_CONTROL_SIZE), (cls, got)
    # the largest valid control with a wrong program: a size that is valid but does not commit
    control = C.seeded_script(s, 33 + 32 * 128)
    got = record("size_128_random", dict(base, control=control), control_seed=[s, 33 + 32 * 128])
    assert got == (0, C.ERR_MISMATCH), got

    # ---- tuples ----
    tuples = []

    def trecord(ts):
        for cls, q, par, p, t in ts:
            tuples.append(dict(cls=cls, q=q.hex(), parity=par, p=p.hex(), t=t.hex(),
                               verdict=T.check(q, par, p, t)))

    edges = C.edge_tuples(rng)
    trecord(edges)
    by = {c["cls"]: c["verdict"] for c in tuples}
    # the issue's table
    for cls, want in (("valid", 1), ("wrong_parity", 0), ("t_zero_par0", 1), ("t_zero_par1", 0),
                      ("t_eq_n", 0), ("t_max", 0), ("t_n_minus_1", 1), ("doubling", 1),
                      ("infinity_q0", 0), ("infinity_qp", 0), ("p_off_curve", 0), ("p_eq_prime", 0),
                      ("p_eq_prime_plus_1", 0), ("parity_2", 0), ("q_plus_1", 0)):
        assert by[cls] == want, (cls, by[cls])
    trecord(C.random_tuples(rng, 120))
    # every edge class inside the inversion groups of a batch of valid rows: groups are strided, so
    # a block of valid rows, one edge row, and so on puts each beside valid neighbours at any stride
    for e in C.edge_tuples(rng):
        trecord([("valid",) + C.valid_tuple(rng) for _ in range(3)])
        trecord([("mix_" + e[0],) + e[1:]])
    trecord([("valid",) + C.valid_tuple(rng) for _ in range(40)])

    doc = dict(spends=spends, tuples=tuples)
    with gzip.GzipFile(C.GOLDEN, "wb", mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    print(f"{len(spends)} spends ({sum(c['ret'] for c in spends)} valid), {len(tuples)} tuples "
          f"({sum(c['verdict'] for c in tuples)} valid), {os.path.getsize(C.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
