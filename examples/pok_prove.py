#!/usr/bin/env python3
"""The prover's side of the reference's examples/pok_sig.rs as ONE call, the counterpart of examples/pok_verify.py.

    prove(cases, ...)                            pok_sig.rs:13-32 for a whole batch: the prover holds (pk, msg, sig) of every case of one
                                                 parameter set.  frw_pok_prove_from_bytes_dev decodes, hashes, screens, makes the
                                                 witnesses and the proofs and encodes them; the prover never sees a witness buffer.  It
                                                 returns ONLY what travels: the verifying key's wire bytes, one status and 192 proof
                                                 bytes per case, and the signatures' 40-byte nonces.  One case is a copy of the first with
                                                 a tampered signature: its status is not 0 and its proof bytes are all zero.
    verify(vk_bytes, pk, nonce, msg, proofs)     pok_sig.rs:33-47, as examples/pok_verify.py: the statements from (pk, nonce, msg) alone
                                                 (Groth16Verifier.verify_statements_wire_dev), the proofs from their wire bytes.

    python examples/pok_prove.py tests/golden/falcon_signed.json [--logn 9] [--seed 1] [--key-file PATH]

--key-file PATH: the proving key is read from PATH if it exists (what pk.serialize(&mut file) wrote), otherwise made and written there.
Exit status 0: every genuine case was proven and its proof accepted, the tampered one was refused by the prover and has no proof.
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


def prove(triples, logn, seed=1, key_file=None):
    """triples: [(pk_bytes, msg, sig_bytes)] -> (vk_bytes, statuses, [proof bytes], [nonce]): what the prover sends"""
    eng = frw.WitnessEngine(0)
    rng = random.Random(seed)
    toxic = [rng.randrange(2, R) for _ in range(5)]
    if key_file and os.path.exists(key_file):
        key, vk = eng.groth16_pk_load_wire(open(key_file, "rb").read())                      # ProvingKey::deserialize: every point checked
    else:
        key, vk = eng.groth16_setup(frw.CIRCUIT_NTT, logn, *toxic)                           # circuit_specific_setup
        if key_file:
            with open(key_file, "wb") as f:
                f.write(eng.groth16_pk_to_wire(key, vk))                                     # pk.serialize(&mut file)
    r1cs = eng.r1cs_load(frw.CIRCUIT_NTT, logn)
    rs = np.frombuffer(b"".join(rng.randrange(R).to_bytes(32, "little") for _ in range(2 * len(triples))), dtype=np.uint64)
    pkb, msgs, sgb = ([t[k] for t in triples] for k in range(3))
    # build_circuit + create_random_proof + Proof::serialize for the batch: two proofs in flight at a time
    out = eng.pok_prove_from_bytes_dev(key, r1cs, frw.CIRCUIT_NTT, logn, pkb, sgb, msgs, rs.reshape(-1, 2, 4), in_flight=2,
                                       want_proofs=False, want_instance=False, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    status = out["status"].tolist()
    wire = out["wire"].cpu().numpy()
    if out["num_unsatisfied"].cpu().numpy().any():
        raise SystemExit("a witness violates its constraint system")
    sent = (frw.vk_to_wire(vk), status, [w.tobytes() for w in wire], [s[1:1 + frw.NONCE_LEN] for s in sgb])
    eng.r1cs_free(r1cs)
    eng.groth16_pk_free(key)
    eng.close()
    return sent


# ------------------------------------------------------------- nothing below this line sees anything of the prover's but prove()'s result
def verify(vk_bytes, logn, pk_bytes, nonces, msgs, proofs):
    """-> (statement statuses FRW_ST_*, verdicts 1 / 0 / -1)"""
    eng = frw.WitnessEngine(0)
    verifier = frw.Groth16Verifier.from_wire(vk_bytes, device=0)                              # VerifyingKey::deserialize: every point checked
    status, verdict = verifier.verify_statements_wire_dev(eng, logn, pk_bytes, nonces, msgs, b"".join(proofs))
    out = status.tolist(), verdict.tolist()                                                   # (the copy to the host waits for the stream)
    verifier.close()
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("signed", help="JSON with cases of {logn, pk_bytes, msg, sig_bytes} (hex)")
    ap.add_argument("--logn", type=int, default=9, choices=(9, 10))
    ap.add_argument("--seed", type=int, default=1, help="seed of the toxic waste and the blinding factors (demonstration only)")
    ap.add_argument("--key-file", help="the proving key in ark-serialize's compressed format: loaded from here if the file exists, else made and saved here")
    args = ap.parse_args()
    cases = [c for c in json.load(open(args.signed))["cases"] if c["logn"] == args.logn]
    if not cases:
        raise SystemExit("no case of logn %d" % args.logn)
    triples = [tuple(bytes.fromhex(c[k]) for k in ("pk_bytes", "msg", "sig_bytes")) for c in cases]
    pkb, msg, sgb = triples[0]
    tampered = len(triples) // 2 + 1                                                          # in the middle of the batch
    triples.insert(tampered, (pkb, msg, sgb[:50] + bytes([sgb[50] ^ 0x40]) + sgb[51:]))
    vk_bytes, status, proofs, nonces = prove(triples, args.logn, args.seed, args.key_file)
    statement, verdict = verify(vk_bytes, args.logn, [t[0] for t in triples], nonces, [t[1] for t in triples], proofs)
    print("Falcon-%d: %d cases in one call, verifying key %d bytes, %d proof bytes each" % (1 << args.logn, len(triples), len(vk_bytes), len(proofs[0])))
    for i, t in enumerate(triples):
        print("  case %d%s (%r): prover status %d, proof %s..., verifier: statement %d, verdict %d"
              % (i, " (tampered)" if i == tampered else "", t[1][:24], status[i], proofs[i][:8].hex(), statement[i], verdict[i]))
    ok = all((status[i] == 0 and verdict[i] == 1) if i != tampered else (status[i] != 0 and not any(proofs[i]) and verdict[i] != 1)
             for i in range(len(triples)))
    if not ok or any(statement):
        raise SystemExit("expected every genuine case proven and accepted, and the tampered one refused")


if __name__ == "__main__":
    main()
