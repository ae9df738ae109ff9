"""Generate tests/golden/taproot_spends.json.gz (run in the build container, where the reference exists).

    python3 tests/golden/make_taproot_spend_fixtures.py

Whole Taproot inputs for bcc_taproot_spend_batch.  The file holds inputs and the REFERENCE's recorded
answers only (oracle/_ref/libref_consensus.so):

  class r_*  spends that reach no Schnorr verification: (ret, serror) of VerifyScript with flags
             0xE15 | 1 << 17 through ref_capture_script;
  class s_*  spends with signatures: the answers of CheckSchnorrSignature (ref_taproot_check) for
             every non-empty signature, in execution order, and the template's arithmetic result
             for the case that all of them pass; the whole-spend expectation is derived from the
             two by tests/taproot_spend_cases.py expected_s (see that module's docstring).

Signatures are made with the reference's secp256k1_schnorrsig_sign over the sighash the reference
computed.  Long scripts and stacks are repetitive, so the gzip stream stays small.
"""
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import taproot_spend_cases as S  # noqa: E402
from oracle_ctypes import Reference  # noqa: E402


def main():
    R = Reference()
    rng = random.Random(0x5BE2D_5EED)
    cases = S.build_class_r(rng) + S.script_bit_cases(R, rng)
    for c in cases:
        c["expected"] = S.ref_whole(R, c)
    by_name = {c["cls"]: c["expected"] for c in cases}
    # the budget cases sit where their names say
    assert by_name["r_weight_exact"] == (1, 0) and by_name["r_weight_annex_pays"] == (1, 0)
    assert by_name["r_weight_one_too_many"] == (0, 48) and by_name["r_weight_annex_one_short"] == (0, 48)
    cases += S.build_class_s(R, rng)
    for _ in range(3):
        cases += S.multi_input_cases(R, rng)
    S.dump_golden(cases)
    errs = {}
    for c in cases:
        errs[c["expected"]] = errs.get(c["expected"], 0) + 1
    print(len(cases), "cases", dict(sorted(errs.items())), os.path.getsize(S.GOLDEN), "bytes")
    missing = S.LISTED_ERRORS - {e for (_, e) in errs}
    assert not missing, missing


if __name__ == "__main__":
    main()
