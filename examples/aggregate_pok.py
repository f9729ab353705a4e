#!/usr/bin/env python3
"""ONE Groth16 proof for several Falcon statements of mixed parameter sets, from their encoded bytes, in ONE call -- both halves of the
reference's examples/pok_sig.rs:21-47 for an aggregate statement (BASELINE configs[4]), the checked counterpart of
examples/aggregate_sig.py, which assembles the same proof by hand from decoded coefficients.

    prove(triples, ...)                          the prover holds (pk, msg, sig) of every statement, in the order of the statement.
                                                 frw_aggregate_prove_from_bytes_dev decodes, hashes, screens every statement, makes the
                                                 witnesses and the one proof and encodes it.  A refused statement means there is no
                                                 proof.  It returns ONLY what travels: the verifying key's wire bytes, the parameter
                                                 sets in order, 192 proof bytes and the signatures' 40-byte nonces.
    verify(vk_bytes, logns, pk, nonce, msg, proof)   the aggregate's public inputs from (pk bytes, nonces, msgs) alone
                                                 (Groth16Verifier.verify_aggregate_wire_dev), the proof from its wire bytes.

    python examples/aggregate_pok.py [tests/golden/falcon_signed.json] [--order 9,10,9] [--seed 1]

Exit status 0: the proof was made in one call, the verifier accepted it, and rejected it with one message byte changed.
"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import falcon_r1cs_amd as frw

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def prove(triples, logns, seed=1):
    """triples: [(pk_bytes, msg, sig_bytes)] in statement order -> (vk_bytes, proof bytes, [nonce]): what the prover sends"""
    eng = frw.WitnessEngine(0)
    rng = random.Random(seed)
    handle = eng.r1cs_load_aggregate(logns)
    key, vk = eng.groth16_setup_r1cs(handle, *(rng.randrange(2, R) for _ in range(5)))          # circuit_specific_setup, for THIS order
    rs = np.frombuffer(b"".join(rng.randrange(R).to_bytes(32, "little") for _ in range(2)), dtype=np.uint64)
    # build_circuit + create_random_proof + Proof::serialize for the whole statement; raises if a statement is refused
    out = eng.aggregate_prove_from_bytes_dev(key, handle, triples, rs, compressed=True, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if out["num_unsatisfied"].tolist() != [0]:
        raise SystemExit("the witness violates the constraint system")
    sent = (frw.vk_to_wire(vk), out["wire"].cpu().numpy().tobytes(), [bytes(n) for n in out["nonces"].cpu().numpy()])
    eng.groth16_pk_free(key)
    eng.r1cs_free(handle)
    eng.close()
    return sent


# ------------------------------------------------------------- nothing below this line sees anything of the prover's but prove()'s result
def verify(vk_bytes, logns, pk_bytes, nonces, msgs, proof):
    """-> (statement statuses FRW_ST_*, verdict 1 / 0 / -1)"""
    eng = frw.WitnessEngine(0)
    handle = eng.r1cs_load_aggregate(logns)                                                    # the statement's shape: public knowledge
    verifier = frw.Groth16Verifier.from_wire(vk_bytes, device=0)                               # VerifyingKey::deserialize: every point checked
    status, verdict = verifier.verify_aggregate_wire_dev(eng, handle, pk_bytes, nonces, msgs, proof)
    out = status.tolist(), verdict.tolist()[0]                                                 # (the copy to the host waits for the stream)
    verifier.close()
    eng.r1cs_free(handle)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("signed", nargs="?", default=os.path.join(ROOT, "tests", "golden", "falcon_signed.json"),
                    help="JSON with cases of {logn, pk_bytes, msg, sig_bytes} (hex)")
    ap.add_argument("--order", default="9,10,9", help="the statements' parameter sets in order; each takes the next unused case of its set")
    ap.add_argument("--seed", type=int, default=1, help="seed of the toxic waste and the blinding factors (demonstration only)")
    args = ap.parse_args()
    logns = [int(x) for x in args.order.split(",")]
    cases = json.load(open(args.signed))["cases"]
    used, triples = {9: 0, 10: 0}, []
    for logn in logns:
        mine = [c for c in cases if c["logn"] == logn]
        if used[logn] >= len(mine):
            raise SystemExit("%s has %d genuine Falcon-%d cases, the order asks for more" % (args.signed, len(mine), 1 << logn))
        c = mine[used[logn]]
        used[logn] += 1
        triples.append(tuple(bytes.fromhex(c[k]) for k in ("pk_bytes", "msg", "sig_bytes")))

    vk_bytes, proof, nonces = prove(triples, logns, args.seed)
    print("one call: %d statements (%s) -> %d proof bytes" % (len(triples), args.order, len(proof)))
    pks, msgs = [t[0] for t in triples], [t[1] for t in triples]
    status, verdict = verify(vk_bytes, logns, pks, nonces, msgs, proof)
    print("verifier, from (pk bytes, nonces, msgs, proof bytes) alone: statuses %s verdict %d -> %s" % (status, verdict, "accepted" if verdict == 1 else "NOT accepted"))
    last = max(i for i, m in enumerate(msgs) if m)                                             # (a message may be empty)
    changed = msgs[:last] + [msgs[last][:-1] + bytes([msgs[last][-1] ^ 1])] + msgs[last + 1:]
    status2, verdict2 = verify(vk_bytes, logns, pks, nonces, changed, proof)
    print("one byte of message %d changed: statuses %s verdict %d -> %s" % (last, status2, verdict2, "rejected" if verdict2 == 0 else "NOT rejected"))
    return 0 if verdict == 1 and not any(status) and verdict2 == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
