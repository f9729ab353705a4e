#!/usr/bin/env python3
"""The verifier's side of the reference's examples/pok_sig.rs, with a hard line between the two parties.

    prove(case)                                  pok_sig.rs:13-32: the prover holds (pk, msg, sig).  It returns ONLY what travels: the
                                                 verifying key's wire bytes, the proof's 192 wire bytes and the signature's 40-byte nonce
                                                 (sig_bytes[1:41]) -- no instance buffer, no signature.
    verify(vk_bytes, pk_bytes, msg, nonce,       pok_sig.rs:33-47: the verifier holds the public key and the message.  It builds the public
           proof_bytes)                          inputs pk_ntt || hm_ntt itself (frw_statement_from_bytes_dev: the key decoder, SHAKE256 and
                                                 the statement kernel on the device) and checks the proof against them
                                                 (frw_groth16_verify_wire_dev).  It touches nothing of the prover's.

    python examples/pok_verify.py tests/golden/falcon_signed.json [--case 0] [--seed 1]

Exit status 0: the genuine statement was accepted and the same proof was rejected for another message.
"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import falcon_r1cs_amd as frw

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def prove(case, seed=1):
    """-> (vk_bytes, proof_bytes, nonce): what the prover sends"""
    logn = case["logn"]
    pk_bytes, msg, sig_bytes = (bytes.fromhex(case[k]) for k in ("pk_bytes", "msg", "sig_bytes"))
    dev = torch.device("cuda:0")
    eng = frw.WitnessEngine(0)
    L = frw.layout(logn)
    sig, pk, hm, st = eng.prepare_inputs(logn, [pk_bytes], [msg], [sig_bytes])
    if st.any():
        raise SystemExit("malformed public key or signature encoding")
    d = [torch.from_numpy(a.view(np.int16)).to(dev) for a in (sig, pk, hm)]
    wit = torch.empty((1, L.num_witness, 4), dtype=torch.int64, device=dev)
    inst = torch.empty((1, L.num_instance, 4), dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    eng.witness_ntt_verify_dev(logn, 1, d[0], d[1], d[2], wit, inst, status, frw.ENC_MONTGOMERY, 0)
    torch.cuda.synchronize()
    if int(status[0]) != 0:
        raise SystemExit("Invalid input: the signature fails its range checks (status %d)" % int(status[0]))
    rng = random.Random(seed)
    key, vk = eng.groth16_setup(0, logn, *(rng.randrange(2, R) for _ in range(5)))           # circuit_specific_setup
    r1cs = eng.r1cs_load(0, logn)
    ws_bytes = eng.groth16_workspace_bytes(key, r1cs, 1)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    proof = torch.empty((1, 48), dtype=torch.int64, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    rs = np.frombuffer(b"".join(rng.randrange(R).to_bytes(32, "little") for _ in range(2)), dtype=np.uint64).reshape(1, 2, 4)
    eng.groth16_prove_dev(key, r1cs, 1, wit, inst, rs, proof, ws, ws_bytes, bad, 0)           # create_random_proof
    torch.cuda.synchronize()
    if int(bad[0]) != 0:
        raise SystemExit("the witness violates %d constraints" % int(bad[0]))
    wire, wire_status = frw.proofs_to_wire_dev(proof)                                         # Proof::serialize
    if int(wire_status[0]) != 0:
        raise SystemExit("the proof does not encode")
    out = (frw.vk_to_wire(vk), wire[0].cpu().numpy().tobytes(), sig_bytes[1:1 + frw.NONCE_LEN])
    eng.r1cs_free(r1cs)
    eng.groth16_pk_free(key)
    eng.close()
    return out


# ------------------------------------------------------------- nothing below this line sees anything of the prover's but prove()'s result
def verify(vk_bytes, pk_bytes, msg, nonce, proof_bytes):
    """-> (statement status FRW_ST_*, verdict 1 / 0 / -1)"""
    logn = {frw.PK_LEN[9]: 9, frw.PK_LEN[10]: 10}[len(pk_bytes)]
    eng = frw.WitnessEngine(0)
    verifier = frw.Groth16Verifier.from_wire(vk_bytes, device=0)                              # VerifyingKey::deserialize: every point checked
    status, verdict = verifier.verify_statements_wire_dev(eng, logn, [pk_bytes], [nonce], [msg], proof_bytes)
    out = int(status[0]), int(verdict[0])                                                     # (the copy to the host waits for the stream)
    verifier.close()
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("signed", help="JSON with cases of {logn, pk_bytes, msg, sig_bytes} (hex)")
    ap.add_argument("--case", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1, help="seed of the toxic waste and the blinding factors (demonstration only)")
    args = ap.parse_args()
    case = json.load(open(args.signed))["cases"][args.case]
    vk_bytes, proof_bytes, nonce = prove(case, args.seed)
    pk_bytes, msg = bytes.fromhex(case["pk_bytes"]), bytes.fromhex(case["msg"])
    genuine = verify(vk_bytes, pk_bytes, msg, nonce, proof_bytes)
    other = verify(vk_bytes, pk_bytes, msg + b"!", nonce, proof_bytes)
    print("verifying key %d bytes, proof %d bytes, nonce %d bytes" % (len(vk_bytes), len(proof_bytes), len(nonce)))
    print("  the statement proved (public key, %r): status %d, verdict %d" % (msg, *genuine))
    print("  another message: status %d, verdict %d" % other)
    if genuine != (0, 1) or other != (0, 0):
        raise SystemExit("expected the genuine statement accepted and the other rejected")


if __name__ == "__main__":
    main()
