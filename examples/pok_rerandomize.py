#!/usr/bin/env python3
"""One proof of knowledge of a signature, presented three times: ark-groth16's rerandomize_proof on the proofs of examples/pok_prove.py.

    prove(...)                                   examples/pok_prove.py: the 192-byte proofs of the golden signatures, one call
    rerandomize(vk_bytes, proofs)                what a HOLDER does before every presentation, or a RELAY before it forwards: from
                                                 (vk, proof bytes) alone -- no signature, no witness, no proving key -- a proof of the
                                                 same statement that shares no point with the one it came from
                                                 (frw_groth16_rerandomize_wire_dev: A' = A / r1, B' = r1 B + r1 r2 delta_g2, C' = C + r2 A).
                                                 The factors come from `secrets`: the new proof is unlinkable to the old one only while
                                                 r1, r2 are uniform, secret and used once.
    verify(...)                                  examples/pok_verify.py's verifier, from (pk, nonce, msg, proof bytes) alone

    python examples/pok_rerandomize.py tests/golden/falcon_signed.json [--logn 9] [--seed 1]

Exit status 0: the verifier accepts the original proofs and both re-randomised sets, and the three sets are pairwise different in every
one of their three points.
"""
import argparse
import json
import os
import secrets
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import falcon_r1cs_amd as frw
import pok_prove

# the compressed proof on the wire: A (48 bytes) | B (96) | C (48)
POINTS = ((0, 48), (48, 144), (144, 192))


def rerandomize(vk_bytes, proofs):
    """[192 proof bytes] -> [192 proof bytes] of the same statements; nothing but the verifying key is needed"""
    dev = torch.device("cuda:0")
    verifier = frw.Groth16Verifier.from_wire(vk_bytes, device=0)
    factors = np.frombuffer(secrets.token_bytes(64 * len(proofs)), dtype=np.uint64).reshape(len(proofs), 2, 4)     # any 256 bits: taken mod r
    d_wire = torch.from_numpy(np.frombuffer(b"".join(proofs), dtype=np.uint8).copy()).to(dev)
    d_factors = torch.from_numpy(factors.view(np.int64).copy()).to(dev)
    out, status = verifier.rerandomize_wire_dev(d_wire, d_factors, stream=torch.cuda.current_stream().cuda_stream)
    status = status.tolist()                                                                   # (the copy to the host waits for the stream)
    if any(status):
        raise SystemExit("a proof was refused: statuses %r" % (status,))
    fresh = [row.tobytes() for row in out.cpu().numpy()]
    verifier.close()
    return fresh


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("signed", help="JSON with cases of {logn, pk_bytes, msg, sig_bytes} (hex)")
    ap.add_argument("--logn", type=int, default=9, choices=(9, 10))
    ap.add_argument("--seed", type=int, default=1, help="seed of the toxic waste and the prover's blinding factors (demonstration only)")
    args = ap.parse_args()
    cases = [c for c in json.load(open(args.signed))["cases"] if c["logn"] == args.logn]
    if not cases:
        raise SystemExit("no case of logn %d" % args.logn)
    triples = [tuple(bytes.fromhex(c[k]) for k in ("pk_bytes", "msg", "sig_bytes")) for c in cases]
    vk_bytes, status, proofs, nonces = pok_prove.prove(triples, args.logn, args.seed)
    if any(status):
        raise SystemExit("the prover refused a genuine case")
    sets = [proofs, rerandomize(vk_bytes, proofs)]
    sets.append(rerandomize(vk_bytes, sets[1]))                                                # a relay re-randomises what it was sent
    ok = True
    for k, name in enumerate(("as proven", "re-randomised", "re-randomised again")):
        statement, verdict = pok_prove.verify(vk_bytes, args.logn, [t[0] for t in triples], nonces, [t[1] for t in triples], sets[k])
        print("%-20s %s  statement %r, verdict %r" % (name, " ".join(p[:6].hex() + ".." for p in sets[k]), statement, verdict))
        ok = ok and not any(statement) and all(v == 1 for v in verdict)
    for i in range(len(triples)):
        for a in range(3):
            for b in range(a + 1, 3):
                ok = ok and all(sets[a][i][lo:hi] != sets[b][i][lo:hi] for lo, hi in POINTS)
    if not ok:
        raise SystemExit("expected all three sets accepted and pairwise different in A, B and C")
    print("three presentations of %d statements, no point in common" % len(triples))


if __name__ == "__main__":
    main()
