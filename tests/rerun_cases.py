"""Verdict-dependent spends: inputs whose later checks depend on an earlier check's verdict, so
that the batch engine needs a second, third or fourth device round for them, and
key-hash spends one bit away from their program.

golden/rerun_cases.json.gz is written by golden/make_rerun_cases.py from build_all() below.  The
builders construct inputs only; every expected value is the reference's (oracle/_ref):
(ret, err) of verify_script_with_amount and, from capture_script, the checks the reference
executed as (sighash, verdict, key, signature) in order.  rounds_min is a lower bound on the device
rounds of the input run alone with every round on the device, taken from the construction (never
from the engine):

  no check executed by the reference (a witness or P2SH wrapping the flag set does not evaluate,
  a failure before the first check)                                   0
  a ladder of depth d                                                 min(d, leading invalid + 1)
  CHECKSIG NOT IF <K> CHECKSIGVERIFY ENDIF 1                          2 if the first is invalid
  the same pair on both sides of OP_CODESEPARATOR, valid after it     2
  m-of-n above the hint bound m (n - m + 1) <= 2 n, every signature and key well formed, and the
  reference executed a pair off the diagonal                          2
  any other input with an executed check that a first run defers (a key of valid length and
  header, a signature that lax DER parses with r, s != 0)              1

The diagonal of a CHECKMULTISIG is the pairs its loop visits while every check succeeds: it starts
at the top of the stack, so signature j of m (in key order) meets key n - m + j first.  A first run
answers every check with a speculative true and therefore defers exactly the diagonal when the
script is above the hint bound; a pair off it is first seen by a re-run.

File layout (everything that repeats is stored once): blobs = hex strings; sighashes = hex; a case
holds spk (blob), tx (list of blobs, concatenated), amount, nin, flags, ret, err, checks
[[sighash, verdict, key blob, signature blob]], family, name, rounds_min, kh (the construction is
a key-hash spend whose first run reaches its signature check through the unrolled P2PKH / P2WPKH
path), group (multi-input: the transaction's tag)."""
import gzip
import hashlib
import json
import os
import struct

from script_asm import hash160, push_data, ser_tx

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "rerun_cases.json.gz")
ALL = 0xE15
FLAG_SETS = (ALL, 0x5, 0)  # VERIFY_ALL, P2SH | DERSIG, NONE
FAMILIES = ("multisig", "ladder", "cache_key", "multi_input", "key_hash")
MN = [(2, 3), (3, 5), (3, 6), (2, 7), (3, 7), (4, 7), (1, 20), (10, 20), (19, 20), (20, 20)]
WRAPPINGS = ("bare", "p2sh", "p2wsh", "p2sh_p2wsh")
MS_OPS = ("cms", "cms_not", "cmsv", "cmsv_not")
KH_KINDS = ("p2wpkh", "p2sh_p2wpkh", "p2pkh")
KEY_FORMS = ("compressed", "uncompressed", "hybrid")

OP_IF, OP_ELSE, OP_ENDIF, OP_DROP, OP_NOT = b"\x63", b"\x67", b"\x68", b"\x75", b"\x91"
OP_CODESEPARATOR, OP_CHECKSIG, OP_CHECKSIGVERIFY = b"\xab", b"\xac", b"\xad"
OP_CHECKMULTISIG, OP_CHECKMULTISIGVERIFY = b"\xae", b"\xaf"


def above_hint_bound(m, n):
    return m * (n - m + 1) > 2 * n


# ---- the loader --------------------------------------------------------------------------------
_cases = None


def load():
    """The cases of the golden file with spk / tx as bytes and checks as dicts."""
    global _cases
    if _cases is None:
        with gzip.open(GOLDEN, "rt") as f:
            d = json.load(f)
        blobs = [bytes.fromhex(b) for b in d["blobs"]]
        shs = [bytes.fromhex(b) for b in d["sighashes"]]
        txs = {}
        out = []
        for c in d["cases"]:
            key = tuple(c["tx"])
            tx = txs.get(key)
            if tx is None:
                tx = txs[key] = b"".join(blobs[i] for i in key)
            c = dict(c, spk=blobs[c["spk"]], tx=tx,
                     checks=[dict(sighash=shs[s], verdict=v, pub=blobs[p], sig=blobs[g])
                             for s, v, p, g in c["checks"]])
            out.append(c)
        _cases = out
    return _cases


def item(c):
    return (c["spk"], c["amount"], c["tx"], c["nin"])


def by_flags(cases):
    out = {}
    for c in cases:
        out.setdefault(c["flags"], []).append(c)
    return out


def selection(cases, every=10):
    """The cases built for a second or later round and every `every`-th of the others."""
    rest = [c for c in cases if c["rounds_min"] < 2]
    ids = {id(c) for c in rest[::every]}
    return [c for c in cases if c["rounds_min"] >= 2 or id(c) in ids]


def thin(cases, every=8):
    """Every multi-input and cache-key case and every `every`-th of the others: the CPU twin's
    shuffled runs under a setting (its device is the plain-C oracle, about 2 ms a check; the whole
    file runs under every setting in file order)."""
    small = ("multi_input", "cache_key")
    rest = [c for c in cases if c["family"] not in small]
    ids = {id(c) for c in rest[::every]}
    return [c for c in cases if c["family"] in small or id(c) in ids]


def lifted(c):
    """(tx, spent outputs, n_in) of a case for bcc_verify_inputs_batch: the case's (amount, spk) at
    nin, OP_RETURN outputs elsewhere (mixed_input_cases.lift)."""
    import mixed_input_cases as M
    return M.case(c["tx"], M.lift(c["spk"], c["amount"], c["tx"], c["nin"]), c["nin"], c["flags"],
                  (c["ret"], c["err"]), "rerun:" + c["name"])


# ---- the writer --------------------------------------------------------------------------------
class Pool:
    """Interns the byte strings that repeat (keys, signatures, scripts): a transaction is stored as
    the list of the registered atoms it contains and the literal bytes between them."""

    def __init__(self):
        self.blobs, self.index = [], {}
        self.shs, self.sh_index = [], {}
        self.atoms = {}  # first 8 bytes -> [atom], longest first

    def atom(self, b):
        if len(b) >= 20:
            lst = self.atoms.setdefault(b[:8], [])
            if b not in lst:
                lst.append(b)
                lst.sort(key=len, reverse=True)
        return b

    def blob(self, b):
        i = self.index.get(b)
        if i is None:
            i = self.index[b] = len(self.blobs)
            self.blobs.append(b)
        return i

    def sighash(self, h):
        i = self.sh_index.get(h)
        if i is None:
            i = self.sh_index[h] = len(self.shs)
            self.shs.append(h)
        return i

    def split(self, tx):
        parts, lit, o = [], bytearray(), 0
        while o < len(tx):
            hit = next((a for a in self.atoms.get(tx[o:o + 8], ()) if tx.startswith(a, o)), None)
            if hit is None:
                lit.append(tx[o])
                o += 1
                continue
            if lit:
                parts.append(self.blob(bytes(lit)))
                lit = bytearray()
            parts.append(self.blob(hit))
            o += len(hit)
        if lit:
            parts.append(self.blob(bytes(lit)))
        assert b"".join(self.blobs[i] for i in parts) == tx
        return parts


# ---- construction ------------------------------------------------------------------------------
def seckey(tag, i):
    return hashlib.sha256(b"rerun %s %d" % (tag.encode(), i)).digest()


def flip_bit(b, bit):
    b = bytearray(b)
    b[bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def pushes(items):
    return b"".join(push_data(x) for x in items)


def small_int(n):
    return bytes([0x50 + n]) if 1 <= n <= 16 else push_data(bytes([n]))


def p2sh(script):
    return b"\xa9\x14" + hash160(script) + b"\x87"


class Ctx:
    """One input of a transaction being signed.  No signature hash of these flag sets covers a
    scriptSig or a witness, so every signature is made over the transaction with both empty."""

    def __init__(self, B, unsigned, nin, amount):
        self.B, self.unsigned, self.nin, self.amount = B, unsigned, nin, amount

    def sign(self, sk, code, sv, ht=1, other_msg=False):
        """A DER signature by sk with hash type ht; other_msg: over another message (well formed,
        invalid for every key)."""
        m = self.B.O.sighash(self.unsigned, self.nin, code, ht, self.amount, sv)
        assert m is not None
        if other_msg:
            m = hashlib.sha256(m).digest()
        return self.B.pool.atom(self.B.R.sign(sk, m) + bytes([ht]))


class Builder:
    def __init__(self, R, O):
        self.R, self.O = R, O
        self.pool = Pool()
        self.cases = []
        self._pubs = {}

    def pub(self, sk, form="compressed"):
        k = (sk, form)
        if k not in self._pubs:
            p = self.R.pubkey_create(sk, form == "compressed")
            if form == "hybrid":  # 0x06 / 0x07 with y's parity (libsecp256k1 parses it)
                p = bytes([6 | (p[64] & 1)]) + p[1:]
            self._pubs[k] = self.pool.atom(p)
        return self._pubs[k]

    # -- wrappings: script + stack items (bottom first) -> (spk, scriptSig, witness) --
    @staticmethod
    def sigversion(wrapping):
        return 1 if wrapping in ("p2wsh", "p2sh_p2wsh") else 0

    def wrap(self, wrapping, script, items):
        self.pool.atom(script)
        if wrapping == "bare":
            return script, pushes(items), []
        if wrapping == "p2sh":
            return p2sh(script), pushes(items) + push_data(script), []
        prog = b"\x00\x20" + hashlib.sha256(script).digest()
        if wrapping == "p2wsh":
            return prog, b"", list(items) + [script]
        return p2sh(prog), push_data(prog), list(items) + [script]

    # -- transactions --
    def transaction(self, tag, specs, amounts):
        """A transaction of len(specs) inputs: specs[k](ctx) -> (spk, scriptSig, witness, info).
        Returns (tx bytes, [(spk, amount, info)])."""
        n = len(specs)
        prev = [hashlib.sha256(b"rerun prevout %s %d" % (tag.encode(), k)).digest() +
                struct.pack("<I", k % 3) for k in range(n)]
        outs = [(amounts[k] - 1000, b"\x51") for k in range(n)]
        unsigned = ser_tx(1, [(p, b"", 0xFFFFFFFF) for p in prev], outs, 0)
        done = [specs[k](Ctx(self, unsigned, k, amounts[k])) for k in range(n)]
        tx = ser_tx(1, [(prev[k], done[k][1], 0xFFFFFFFF) for k in range(n)], outs, 0,
                    [d[2] for d in done])
        return tx, [(d[0], amounts[k], d[3]) for k, d in enumerate(done)]

    def single(self, family, name, tag, spec, amount=250000):
        tx, ins = self.transaction(tag, [spec], [amount])
        self.emit(family, name, ins[0][0], amount, tx, 0, ins[0][2])

    def emit(self, family, name, spk, amount, tx, nin, info, group=None):
        parts = self.pool.split(tx)
        for flags in FLAG_SETS:
            ret, err = self.R.verify_script_with_amount(spk, amount, tx, nin, flags)
            r2, _, recs = self.R.capture_script(spk, amount, tx, nin, flags, cap=64)
            assert r2 == ret and len(recs) < 64, (name, flags, ret, r2)
            c = dict(family=family, name=name, spk=self.pool.blob(spk), amount=amount, tx=parts,
                     nin=nin, flags=flags, ret=ret, err=err,
                     checks=[[self.pool.sighash(r["sighash"]), r["verdict"], self.pool.blob(r["pub"]),
                              self.pool.blob(r["sig"])] for r in recs],
                     rounds_min=rounds_model(info, recs, self.O),
                     kh=int(bool(info.get("kh")) and key_hash_first_run(info, flags)))
            if group is not None:
                c["group"] = group
            self.cases.append(c)

    def dump(self):
        return dict(blobs=[b.hex() for b in self.pool.blobs],
                    sighashes=[h.hex() for h in self.pool.shs], cases=self.cases)


def first_run_defers(O, rec):
    """Whether a check the reference executed goes to the device (the host decides a
    key of bad length or header, a signature lax DER does not parse, r = 0 and s = 0; the reference
    records no check of an empty signature).  By the oracle's parsers."""
    pub = rec["pub"]
    if not ((len(pub) == 33 and pub[0] in (2, 3)) or (len(pub) == 65 and pub[0] in (4, 6, 7))):
        return False
    ok, r, s = O.der_parse_lax(rec["sig"])
    return bool(ok) and any(r) and any(s)


def rounds_model(info, recs, O):
    """rounds_min of the module docstring.  recs: the reference's executed checks.  The checks
    before the first one that a first run defers are decided on the host as the reference decides
    them, so a first run reaches that check and needs a device round for it."""
    if not recs:
        return 0
    kind = info["kind"]
    if kind == "ladder":
        return min(info["depth"], info["leading_invalid"] + 1)
    if kind == "fixed":
        return info["rounds"]
    if kind == "multisig" and above_hint_bound(info["m"], info["n"]) and info["well_formed"]:
        m, n, pubs, sigs = info["m"], info["n"], info["pubs"], info["sigs"]
        sigs = [s[:-1] for s in sigs]  # the records hold the signature without its hash type
        if any(pubs.index(r["pub"]) != n - m + sigs.index(r["sig"]) for r in recs):
            return 2
    return 1 if any(first_run_defers(O, r) for r in recs) else 0


def key_hash_first_run(info, flags):
    """Whether the first run of a key-hash construction reaches its signature check through the
    unrolled path that can hand the hash comparison to the device: the wrapping is evaluated under
    the flag set, the signature passes the DER rule, and a P2PKH stack holds at most 100 elements."""
    kind = info["kh"]
    if kind == "p2pkh":
        return info["extra"] + 2 <= 100
    return flags & 0x800 != 0  # WITNESS (which implies P2SH here)


# ---- family: CHECKMULTISIG ---------------------------------------------------------------------
def signer_sets(m, n):
    """first m, last m, alternating (every other key while m allows it); equal sets once."""
    out = {}
    for name, ks in (("first", list(range(m))), ("last", list(range(n - m, n))),
                     ("alt", sorted({i * n // m for i in range(m)}))):
        if ks not in out.values():
            out[name] = ks
    return out


MS_VARIANTS = ("valid", "inv_first", "inv_mid", "inv_last", "swap", "repeat", "outside", "empty",
               "nonder", "badkey_header", "badkey_length", "hashtypes")
HASH_TYPES = (1, 2, 3, 0x81, 0x82, 0x83)


def nonder(sig):
    """The same r and s with r padded by a zero byte: lax DER parses it, BIP66 refuses it."""
    assert sig[0] == 0x30 and sig[2] == 0x02
    rl = sig[3]
    return bytes([0x30, sig[1] + 1, 0x02, rl + 1, 0x00]) + sig[4:]


def multisig_spec(B, m, n, signers, variant, op, wrapping):
    def spec(ctx):
        sks = [seckey("ms%d" % n, i) for i in range(n)]
        pubs = [B.pub(sk) for sk in sks]
        mid_key = n // 2
        if variant == "badkey_header":
            pubs[mid_key] = bytes([5]) + pubs[mid_key][1:]
        if variant == "badkey_length":
            pubs[mid_key] = pubs[mid_key][:32]
        script = small_int(m) + pushes(pubs) + small_int(n)
        script += OP_CHECKMULTISIGVERIFY if op.startswith("cmsv") else OP_CHECKMULTISIG
        if op.endswith("_not"):
            script += OP_NOT
        sv = B.sigversion(wrapping)
        hts = [HASH_TYPES[j % 6] if variant == "hashtypes" else 1 for j in range(m)]
        sigs = [ctx.sign(sks[k], script, sv, hts[j]) for j, k in enumerate(signers)]
        mid = m // 2
        pos = {"inv_first": 0, "inv_mid": mid, "inv_last": m - 1}.get(variant)
        if pos is not None:
            sigs[pos] = ctx.sign(sks[signers[pos]], script, sv, other_msg=True)
        elif variant == "swap" and m >= 2:
            sigs[0], sigs[m - 1] = sigs[m - 1], sigs[0]
        elif variant == "repeat" and m >= 2:
            sigs[m - 1] = sigs[0]
        elif variant == "outside":
            sigs[mid] = ctx.sign(seckey("outside", n), script, sv)
        elif variant == "empty":
            sigs[mid] = b""
        elif variant == "nonder":
            sigs[mid] = B.pool.atom(nonder(sigs[mid]))
        items = ([b"\x01"] if op.startswith("cmsv") else []) + [b""] + sigs
        spk, ss, wit = B.wrap(wrapping, script, items)
        well_formed = variant in ("valid", "inv_first", "inv_mid", "inv_last", "swap", "outside",
                                  "hashtypes")
        return spk, ss, wit, dict(kind="multisig", m=m, n=n, pubs=pubs, sigs=sigs,
                                  well_formed=well_formed)
    return spec


def build_multisig(B):
    rot = 0
    for m, n in MN:
        wraps = [w for w in WRAPPINGS if not (w == "p2sh" and n == 20)]  # 20 keys exceed a P2SH push
        for sname, signers in signer_sets(m, n).items():
            for variant in MS_VARIANTS:
                if m < 2 and variant in ("swap", "repeat"):
                    continue
                if variant == "valid":
                    combos = [(op, w) for w in wraps for op in (MS_OPS if n < 20 else MS_OPS[:1])]
                    if n == 20:
                        combos += [(op, wraps[(rot + i) % len(wraps)]) for i, op in enumerate(MS_OPS[1:])]
                else:
                    # one opcode form and wrapping per variant, rotating through all of them
                    k = 2 if n < 20 else 1
                    combos = [(MS_OPS[(rot + i) % 4], wraps[(rot // 4 + i) % len(wraps)])
                              for i in range(k)]
                rot += 1
                for op, w in combos:
                    tag = "ms %d %d %s" % (m, n, sname)
                    B.single("multisig", "%dof%d:%s:%s:%s:%s" % (m, n, sname, variant, op, w), tag,
                             multisig_spec(B, m, n, signers, variant, op, w))


# ---- family: ladders ---------------------------------------------------------------------------
def ladder_script(pubs):
    s = b"\x00"
    for p in reversed(pubs):
        s = push_data(p) + OP_CHECKSIG + OP_IF + b"\x51" + OP_ELSE + s + OP_ENDIF
    return s


def ladder_spec(B, depth, pattern, wrapping, form="compressed"):
    """<K0> CHECKSIG IF 1 ELSE <K1> CHECKSIG IF 1 ELSE ... 0 ENDIF ... ENDIF with one signature per
    key, the one for K0 on top; bit k of pattern: the signature for key k is valid."""
    def spec(ctx):
        sks = [seckey("ladder", i) for i in range(depth)]
        script = ladder_script([B.pub(sk, form) for sk in sks])
        sv = B.sigversion(wrapping)
        valid = [bool(pattern >> k & 1) for k in range(depth)]
        sigs = [ctx.sign(sks[k], script, sv, other_msg=not valid[k]) for k in range(depth)]
        lead = next((k for k in range(depth) if valid[k]), depth)
        spk, ss, wit = B.wrap(wrapping, script, sigs[::-1])
        return spk, ss, wit, dict(kind="ladder", depth=depth, leading_invalid=lead)
    return spec


def not_if_spec(B, pattern, wrapping):
    """<K0> CHECKSIG NOT IF <K1> CHECKSIGVERIFY ENDIF 1"""
    def spec(ctx):
        sks = [seckey("notif", i) for i in range(2)]
        script = (push_data(B.pub(sks[0])) + OP_CHECKSIG + OP_NOT + OP_IF + push_data(B.pub(sks[1])) +
                  OP_CHECKSIGVERIFY + OP_ENDIF + b"\x51")
        sv = B.sigversion(wrapping)
        sigs = [ctx.sign(sks[k], script, sv, other_msg=not (pattern >> k & 1)) for k in range(2)]
        spk, ss, wit = B.wrap(wrapping, script, sigs[::-1])
        return spk, ss, wit, dict(kind="fixed", rounds=1 if pattern & 1 else 2)
    return spec


def build_ladders(B):
    for wrapping in ("bare", "p2wsh"):
        for form in ("compressed", "uncompressed"):
            for depth in range(1, 5):
                for pattern in range(1 << depth):
                    B.single("ladder", "ladder:%d:%s:%s:%s" % (depth, format(pattern, "0%db" % depth),
                                                              wrapping, form),
                             "ladder %d" % depth, ladder_spec(B, depth, pattern, wrapping, form))
        for pattern in range(4):
            B.single("ladder", "notif:%s:%s" % (format(pattern, "02b"), wrapping), "notif",
                     not_if_spec(B, pattern, wrapping))


# ---- family: the cache key ---------------------------------------------------------------------
def twice_spec(B, valid):
    """<K> CHECKSIGVERIFY <K> CHECKSIG under the same signature twice (bare, legacy)."""
    def spec(ctx):
        sk = seckey("twice", 0)
        k = push_data(B.pub(sk))
        script = k + OP_CHECKSIGVERIFY + k + OP_CHECKSIG
        sig = ctx.sign(sk, script, 0, other_msg=not valid)
        return script, pushes([sig, sig]), [], dict(kind="plain")
    return spec


def codesep_spec(B, first_valid):
    """The same (signature, key) on both sides of an OP_CODESEPARATOR in a legacy script: the
    scriptCode of the first check is the whole script, of the second what follows the separator.
    first_valid: <K> CHECKSIGVERIFY CODESEPARATOR <K> CHECKSIG under a signature for the first
    scriptCode (invalid: the second check fails); else <K> CHECKSIG NOT VERIFY CODESEPARATOR <K>
    CHECKSIG under a signature for the second (valid, and the second check is first met by the
    re-run that knows the first one failed)."""
    def spec(ctx):
        sk = seckey("codesep", 0)
        k = push_data(B.pub(sk))
        tail = k + OP_CHECKSIG
        if first_valid:
            script = k + OP_CHECKSIGVERIFY + OP_CODESEPARATOR + tail
            sig = ctx.sign(sk, script, 0)
        else:
            script = k + OP_CHECKSIG + OP_NOT + b"\x69" + OP_CODESEPARATOR + tail
            sig = ctx.sign(sk, tail, 0)
        return script, pushes([sig, sig]), [], dict(kind="fixed", rounds=1 if first_valid else 2)
    return spec


def find_and_delete_spec(B, valid, deleted):
    """A legacy scriptPubKey that holds the signature's own push: <sig> DROP <K> CHECKSIG, signed
    over the script FindAndDelete leaves (deleted); or the push of another signature, which stays."""
    def spec(ctx):
        sk = seckey("fad", 0)
        tail = OP_DROP + push_data(B.pub(sk)) + OP_CHECKSIG
        if not deleted:  # the push of another signature: nothing is deleted
            script = push_data(ctx.sign(sk, tail, 0, ht=2)) + tail
            sig = ctx.sign(sk, script, 0, other_msg=not valid)
            return script, pushes([sig]), [], dict(kind="plain")
        sig = ctx.sign(sk, tail, 0, other_msg=not valid)
        return push_data(sig) + tail, pushes([sig]), [], dict(kind="plain")
    return spec


def build_cache_key(B):
    for v in (True, False):
        B.single("cache_key", "twice:%d" % v, "twice", twice_spec(B, v))
        B.single("cache_key", "codesep:first_valid=%d" % v, "codesep", codesep_spec(B, v))
        for d in (True, False):
            B.single("cache_key", "find_and_delete:valid=%d:deleted=%d" % (v, d), "fad",
                     find_and_delete_spec(B, v, d))


# ---- family: key-hash near misses --------------------------------------------------------------
def key_hash_spec(B, kind, form, bit=None, bad_sig=False, extra=0, key=0):
    """A P2WPKH / P2SH-P2WPKH / P2PKH spend signed for the scriptCode of its own program.  bit: the
    program is HASH160(key) with that bit flipped (the signature stays valid for the key);
    bad_sig: the signature is over another message; extra: pushes under (sig, key) in a P2PKH
    scriptSig."""
    def spec(ctx):
        sk = seckey("kh " + form, key)
        pub = B.pub(sk, form)
        prog = hash160(pub)
        if bit is not None:
            prog = flip_bit(prog, bit)
        code = b"\x76\xa9\x14" + prog + b"\x88\xac"
        info = dict(kind="plain", kh=kind, extra=extra)
        if kind == "p2pkh":
            sig = ctx.sign(sk, code, 0, other_msg=bad_sig)
            return code, b"\x51" * extra + pushes([sig, pub]), [], info
        sig = ctx.sign(sk, code, 1, other_msg=bad_sig)
        wprog = b"\x00\x14" + prog
        if kind == "p2wpkh":
            return wprog, b"", [sig, pub], info
        return p2sh(wprog), push_data(wprog), [sig, pub], info
    return spec


def build_key_hash(B):
    for kind in KH_KINDS:
        for form in KEY_FORMS:
            tag = "kh %s %s" % (kind, form)
            for bad_sig in (False, True):
                B.single("key_hash", "%s:%s:right:badsig=%d" % (kind, form, bad_sig), tag,
                         key_hash_spec(B, kind, form, None, bad_sig))
                B.single("key_hash", "%s:%s:bit7:badsig=%d" % (kind, form, bad_sig), tag + " w",
                         key_hash_spec(B, kind, form, 7, bad_sig, key=1))
            for bit in range(160):
                B.single("key_hash", "%s:%s:sweep:%d" % (kind, form, bit), tag + " s",
                         key_hash_spec(B, kind, form, bit, key=2))
    for extra in (1, 98, 99):
        for bit in (None, 0):
            B.single("key_hash", "p2pkh:compressed:extra%d:%s" % (extra, "right" if bit is None else "bit0"),
                     "kh extra", key_hash_spec(B, "p2pkh", "compressed", bit, extra=extra, key=3))


# ---- family: multi-input transactions ----------------------------------------------------------
def build_multi_input(B):
    """Transactions of 2-6 inputs drawn from the families above and plain valid key-hash spends, so
    that after the first round only some inputs of a transaction re-run.  Each is built twice:
    'full' has every input as a case (adjacent items on one tx buffer in file order), 'subset'
    only every other input."""
    def pool(k):
        return [
            key_hash_spec(B, "p2wpkh", "compressed", key=10 + k),
            ladder_spec(B, 3, 0b100, "bare"),                                # 3 rounds
            key_hash_spec(B, "p2pkh", "uncompressed", key=10 + k),
            # 2 rounds, and the re-run's BIP143 aux messages (six hash types) are not round 1's
            multisig_spec(B, 4, 7, [0, 1, 2, 3], "hashtypes", "cms", "p2wsh"),
            ladder_spec(B, 4, 0b1000, "p2wsh"),                              # 4 rounds
            multisig_spec(B, 2, 3, [0, 2], "inv_last", "cms", "p2sh"),       # hinted: 1 round
            not_if_spec(B, 0b10, "p2wsh"),                                   # 2 rounds
            key_hash_spec(B, "p2sh_p2wpkh", "compressed", bit=159, key=10 + k),
            ladder_spec(B, 2, 0b00, "bare"),                                 # 2 rounds, invalid
            multisig_spec(B, 3, 7, [0, 2, 4], "hashtypes", "cmsv", "p2sh_p2wsh"),
        ][k % 10]
    t = 0
    for n in range(2, 7):
        for start in (0, 3, 7):
            specs = [pool(start + k) for k in range(n)]
            amounts = [300000 + 17 * (start + k) for k in range(n)]
            for variant in ("full", "subset"):
                tag = "multi %d %d %s" % (n, start, variant)
                tx, ins = B.transaction(tag, specs, amounts)
                for k, (spk, amount, info) in enumerate(ins):
                    if variant == "subset" and k % 2 == 0 and n > 2:
                        continue
                    if variant == "subset" and n == 2 and k == 0:
                        continue
                    B.emit("multi_input", "multi:%d:%d:%s:in%d" % (n, start, variant, k), spk,
                           amount, tx, k, info, group=t)
                t += 1


def build_all(R, O):
    B = Builder(R, O)
    build_multisig(B)
    build_ladders(B)
    build_cache_key(B)
    build_multi_input(B)
    build_key_hash(B)
    return B.dump()


def dumps(d):
    """The golden file's bytes: compact JSON, gzip with no name and no time (regenerates byte for
    byte)."""
    import io
    raw = json.dumps(d, separators=(",", ":"), sort_keys=True).encode()
    buf = io.BytesIO()
    with gzip.GzipFile(filename="", mode="wb", fileobj=buf, mtime=0, compresslevel=9) as g:
        g.write(raw)
    return buf.getvalue()
