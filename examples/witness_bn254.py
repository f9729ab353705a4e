#!/usr/bin/env python3
"""The witness of the reference's verification circuit for a host whose SNARK field is NOT BLS12-381's: every circuit of the
reference is `impl<F: PrimeField> ConstraintSynthesizer<F>` (falcon_ntt.rs:20), and this is F = BN254's Fr -- the field of
every Ethereum-verifiable Groth16, of snarkjs and of gnark.

    python examples/witness_bn254.py tests/golden/falcon_signed.json [--case 0]

A genuine Falcon-512 signature: encoded (public key, message, signature) -> decoders and SHAKE256 on the device -> the modulus
registered on the context (frw_ctx_field_encoding) -> frw_witness_ntt_verify with the encoding that came back: witness_assignment
and instance_assignment in ark-ff's Montgomery bytes over BN254, x * 2^256 mod p.  Checked here against the arkworks front-end
simulation run over that field (oracle/ark_sim.ConstraintSystem(p) with oracle/falcon_gadgets): same values element by element,
and the system they belong to is satisfied.

Exit status 0: the bytes are the oracle's and the oracle's system is satisfied.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import falcon_r1cs_amd as frw

BN254_FR = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


def to_ints(a):
    return [int.from_bytes(r.tobytes(), "little") for r in np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("signed", help="JSON with cases of {logn, pk_bytes, msg, sig_bytes} (hex)")
    ap.add_argument("--case", type=int, default=0, help="which of the Falcon-512 cases")
    args = ap.parse_args()
    case = [c for c in json.load(open(args.signed))["cases"] if c["logn"] == 9][args.case]
    p = BN254_FR
    info = frw.field_info(p)
    print("BN254 Fr: %d bits, one = 2^256 mod p = 0x%064x, -p^-1 mod 2^32 = 0x%08x" % (info.bits, info.one, info.ninv32))

    eng = frw.WitnessEngine(0)
    sig, pk, hm, st = eng.prepare_inputs(9, [bytes.fromhex(case["pk_bytes"])], [bytes.fromhex(case["msg"])], [bytes.fromhex(case["sig_bytes"])])
    if st.any():
        raise SystemExit("the encoded inputs were refused: status %s" % st.tolist())
    enc = eng.field_encoding(p)
    wit, inst, st = eng.witness_ntt_verify(9, sig, pk, hm, enc, strict=True)
    eng.close()
    print("encoding %d: witness %s, instance %s, status %s" % (enc, wit.shape, inst.shape, st.tolist()))

    from oracle import falcon_gadgets as G
    from oracle.ark_sim import ConstraintSystem
    cs = ConstraintSystem(p)
    G.FalconNTTVerificationCircuit(sig[0].tolist(), pk[0].tolist(), hm[0].tolist(), 9).generate_constraints(cs, strict=True)
    mont = lambda v: v * info.one % p
    same = to_ints(wit[0]) == [mont(v) for v in cs.witness_assignment] and to_ints(inst[0]) == [mont(v) for v in cs.instance_assignment]
    satisfied = cs.is_satisfied()
    print("oracle over BN254: %d witness and %d instance variables, %d constraints, satisfied: %s, bytes equal: %s"
          % (cs.num_witness_variables(), cs.num_instance_variables(), cs.num_constraints(), satisfied, same))
    if not (same and satisfied):
        raise SystemExit("the witness over BN254 is not the oracle's")


if __name__ == "__main__":
    main()
