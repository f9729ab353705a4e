#!/usr/bin/env python3
"""Fresh proofs without minting factors on the host: one secret seed and one counter in device memory, and every call draws its own
blinding or re-randomising factors there (frw.h, "drawing the factors on the device").

The statement is the cubic system of examples/custom_r1cs.py (x^3 + x + 5 = y, y public; I = 2, W = 3, C = 3, the 2^3 domain).
    seed = secrets.token_bytes(32), uploaded once; counter = 0 in device memory
    groth16_prove_seeded_dev three times        -> three proofs of the same statement with no point in common, each accepted
    rerandomize_wire_seeded_dev twice           -> two more presentations of the first proof, no point in common, each accepted
Nothing crosses the host boundary between the calls: the counter advances on the device.  The prover is called three times rather than
captured once and replayed: a captured prover is established for the Falcon circuits' keys (tests/test_gpu_drbg.py replays one), not
yet for a 2^3 domain.

The seed is the secret: whoever knows (seed, counter) knows every factor.  A real prover persists the counter ahead of its use or, as
here, takes a new seed from the operating system on every start.

    python examples/pok_fresh_proofs.py [--x 3]

Exit status 0 only when all five proofs are accepted, none is accepted for y + 1, and no two share a point.
"""
import argparse
import os
import random
import secrets
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import falcon_r1cs_amd as frw
from custom_r1cs import R, montgomery, write_r1cs

POINTS = ((0, 48), (48, 144), (144, 192))        # A | B | C in a compressed proof


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--x", type=int, default=3, help="the secret")
    args = ap.parse_args()
    ONE, Y, X, X2, X3 = range(5)
    a = [[(1, X)], [(1, X2)], [(1, X3), (1, X), (5, ONE)]]
    b = [[(1, X)], [(1, X)], [(1, ONE)]]
    c = [[(1, X2)], [(1, X3)], [(1, Y)]]
    x = args.x % R
    y = (x ** 3 + x + 5) % R
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    eng = frw.WitnessEngine(0)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cubic.r1cs")
        write_r1cs(path, 2, 3, (a, b, c))
        r1cs = eng.r1cs_load_file(path)
    toxic = random.Random(1)                         # (demonstration only: a key whose toxic waste is known proves nothing to anyone else)
    key, vk = eng.groth16_setup_r1cs(r1cs, *(toxic.randrange(2, R) for _ in range(5)))
    verifier = frw.Groth16Verifier.from_wire(frw.vk_to_wire(vk), device=0)
    wit = montgomery([x, x * x, x ** 3]).to(dev)
    inst = montgomery([1, y]).to(dev)
    wrong = montgomery([1, y + 1]).to(dev)

    # the only secret, and the only bytes that cross the host boundary: 32 from the operating system's generator
    d_seed = torch.from_numpy(np.frombuffer(secrets.token_bytes(32), dtype=np.uint8).copy()).to(dev)
    d_counter = torch.zeros(1, dtype=torch.int64, device=dev)

    ws_bytes = eng.groth16_workspace_bytes(key, r1cs, 1)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    d_rs = torch.empty((1, 2, 4), dtype=torch.int64, device=dev)
    proof = torch.empty((1, 48), dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    wires = []
    for k in range(3):
        eng.groth16_prove_seeded_dev(key, r1cs, 1, wit, inst, d_seed, d_counter, d_rs, proof, ws, ws_bytes, bad, stream)
        wire, status = frw.proofs_to_wire_dev(proof, stream=stream)
        if bad.tolist() != [0] or status.tolist() != [0]:
            raise SystemExit("the witness does not satisfy the system")
        wires.append(wire.reshape(-1).clone())
    for k in range(2):
        fresh, status, _ = verifier.rerandomize_wire_seeded_dev(wires[0], d_seed, d_counter, stream=stream)
        if status.tolist() != [0]:
            raise SystemExit("re-randomisation refused (status %s)" % status.tolist())
        wires.append(fresh.reshape(-1).clone())

    ok = True
    for k, w in enumerate(wires):
        accepted = verifier.verify_wire_dev(inst, w, stream=stream).tolist() == [1]
        refused = verifier.verify_wire_dev(wrong, w, stream=stream).tolist() == [0]
        print("%s %d: %s  accepted: %s, for y + 1: %s" % ("proof" if k < 3 else "re-randomised", k if k < 3 else k - 3,
                                                          w.cpu().numpy().tobytes().hex()[:32] + "...", accepted, not refused))
        ok = ok and accepted and refused
    raw = [w.cpu().numpy().tobytes() for w in wires]
    distinct = all(len({r[lo:hi] for r in raw}) == len(raw) for lo, hi in POINTS)
    counter = int(d_counter.cpu()[0])
    print("no point in common: %s; the device counter reads %d after five calls" % (distinct, counter))
    verifier.close()
    eng.groth16_pk_free(key)
    eng.r1cs_free(r1cs)
    eng.close()
    if not ok or not distinct or counter != 5:
        raise SystemExit("expected five accepted proofs with no point in common and a counter of 5")


if __name__ == "__main__":
    main()
