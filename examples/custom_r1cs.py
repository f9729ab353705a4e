#!/usr/bin/env python3
"""Groth16 for a constraint system of your own: the textbook x^3 + x + 5 = y with y public.

    I = 2   instance variables: column 0 the constant one, column 1 the public y
    W = 3   witness variables:  column 2 x, column 3 x^2, column 4 x^3
    C = 3   constraints:        x * x = x^2;   x^2 * x = x^3;   (x^3 + x + 5) * 1 = y          QAP domain: next_power_of_two(3 + 2) = 2^3

The system is written as an FRWR1CS1 file (the layout frw_r1cs_export writes: include/frw.h), then
    r1cs_load_file -> groth16_setup_r1cs -> groth16_prove_dev -> proofs_to_wire_dev -> verify_wire_dev (the verifier made from the key's
    wire bytes) -> rerandomize_wire_dev -> verify_wire_dev
all on device 0.  A Rust host passes ark-relations' cs.to_matrices() to frw_r1cs_load_csr instead of writing a file.

    python examples/custom_r1cs.py [--x 3] [--seed 1]

Prints `accepted: True` for y = x^3 + x + 5 and `accepted: False` for y + 1; exit status 0 when both are as expected and the
re-randomised proof is accepted too.
"""
import argparse
import os
import random
import secrets
import struct
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import falcon_r1cs_amd as frw

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001         # the group order: BLS12-381's scalar field


def write_r1cs(path, num_instance, num_witness, matrices):
    """matrices: A, B, C as lists of rows of (coefficient, column) -> the FRWR1CS1 file"""
    with open(path, "wb") as f:
        f.write(b"FRWR1CS1")
        f.write(struct.pack("<6Q", num_instance, num_witness, len(matrices[0]), *(sum(len(r) for r in m) for m in matrices)))
        for m in matrices:
            ptr = [0]
            for row in m:
                ptr.append(ptr[-1] + len(row))
            f.write(struct.pack("<%dQ" % len(ptr), *ptr))
            f.write(struct.pack("<%dI" % ptr[-1], *(col for row in m for _, col in row)))
            f.write(b"".join((coeff % R).to_bytes(32, "little") for row in m for coeff, _ in row))


def montgomery(values):
    """integers -> ark-ff's bytes (x 2^256 mod r, little-endian limbs) as an int64 tensor [1, len, 4]"""
    raw = b"".join((v % R * (1 << 256) % R).to_bytes(32, "little") for v in values)
    return torch.from_numpy(np.frombuffer(raw, dtype=np.int64).reshape(1, len(values), 4).copy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--x", type=int, default=3, help="the secret")
    ap.add_argument("--seed", type=int, default=1, help="seed of the toxic waste and the blinding factors (demonstration only)")
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
    info = eng.r1cs_info(r1cs)
    print("I = %d, W = %d, C = %d, domain 2^%d" % (info.num_instance, info.num_witness, info.num_constraints, info.log_domain_size))
    rng = random.Random(args.seed)
    key, vk = eng.groth16_setup_r1cs(r1cs, *(rng.randrange(2, R) for _ in range(5)))
    wit = montgomery([x, x * x, x ** 3]).to(dev)
    inst = montgomery([1, y]).to(dev)
    ws_bytes = eng.groth16_workspace_bytes(key, r1cs, 1)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    proofs = torch.empty((1, 48), dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    rs = np.frombuffer(b"".join(rng.randrange(R).to_bytes(32, "little") for _ in range(2)), dtype=np.uint64).reshape(1, 2, 4)
    eng.groth16_prove_dev(key, r1cs, 1, wit, inst, rs, proofs, ws, ws_bytes, bad, stream)
    wire, status = frw.proofs_to_wire_dev(proofs, stream=stream)
    if bad.tolist() != [0] or status.tolist() != [0]:
        raise SystemExit("the witness does not satisfy the system")
    print("proof: %s" % wire[0].cpu().numpy().tobytes().hex())
    # the verifier: the key's wire bytes, the public input, the proof's wire bytes
    verifier = frw.Groth16Verifier.from_wire(frw.vk_to_wire(vk), device=0)
    accepted = verifier.verify_wire_dev(inst, wire.reshape(-1), stream=stream).tolist() == [1]
    print("accepted: %s" % accepted)
    wrong = verifier.verify_wire_dev(montgomery([1, y + 1]).to(dev), wire.reshape(-1), stream=stream).tolist() == [1]
    print("accepted: %s" % wrong)
    factors = torch.from_numpy(np.frombuffer(secrets.token_bytes(64), dtype=np.int64).reshape(1, 2, 4).copy()).to(dev)
    fresh, status = verifier.rerandomize_wire_dev(wire.reshape(-1), factors, stream=stream)
    again = status.tolist() == [0] and verifier.verify_wire_dev(inst, fresh.reshape(-1), stream=stream).tolist() == [1]
    print("re-randomised: accepted: %s, shares a point: %s" % (again, any(bool((fresh[0, lo:hi] == wire[0, lo:hi]).all()) for lo, hi in ((0, 48), (48, 144), (144, 192)))))
    verifier.close()
    eng.groth16_pk_free(key)
    eng.r1cs_free(r1cs)
    eng.close()
    if not accepted or wrong or not again:
        raise SystemExit("expected the proof accepted for y, refused for y + 1, and accepted again once re-randomised")


if __name__ == "__main__":
    main()
