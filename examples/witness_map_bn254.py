#!/usr/bin/env python3
"""`R1CStoQAP::witness_map`, the first step of Groth16::prove, for a host whose SNARK field is BN254's Fr, on the device.

    python examples/witness_map_bn254.py [tests/golden/falcon_signed.json] [--case 0]

A genuine Falcon-512 signature: encoded (public key, message, signature) -> decoders and SHAKE256 on the device -> the witness over
BN254 (frw_ctx_field_encoding, frw_witness_ntt_verify_dev) -> frw_qapf_witness_map_dev: the coefficients of
h(X) = (A(X) B(X) - C(X)) / (X^n - 1) over BN254's radix-2 domain of 2^17 points, the coset by ark-bn254's generator 5.  Then the
defining identity is checked here without any FFT, in Python integers: with A z, B z, C z from frw_r1csf_check_dev and L_i the
Lagrange basis of the domain, A(t) B(t) - C(t) = h(t) (t^n - 1) at two random points t.

Exit status 0: 0 violated rows, h of degree < n - 1, and the identity holds at both points.
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

BN254_FR = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
GENERATOR = 5           # ark-bn254's FrParameters::GENERATOR


def to_ints(t):
    return [int.from_bytes(r.tobytes(), "little") for r in np.ascontiguousarray(t.cpu().numpy()).view(np.uint64).reshape(-1, 4)]


def identity_sides(p, dom, rows_a, rows_b, rows_c, h, t):
    """(A(t) B(t) - C(t), h(t) (t^n - 1)) with A(t) = sum a_i L_i(t), L_i(t) = (t^n - 1) w^i / (n (t - w^i))"""
    n = dom.size
    zt = (pow(t, n, p) - 1) % p
    points, w = [], 1
    for _ in range(max(len(rows_a), len(rows_b), len(rows_c))):
        points.append(w)
        w = w * dom.group_gen % p
    prefix, acc = [], 1                                      # one inversion for all the denominators
    for x in points:
        prefix.append(acc)
        acc = acc * ((t - x) % p) % p
    inv, lag = pow(acc, p - 2, p), [0] * len(points)
    for i in range(len(points) - 1, -1, -1):
        lag[i] = inv * prefix[i] % p * points[i] % p * zt % p * dom.size_inv % p
        inv = inv * ((t - points[i]) % p) % p
    at, bt, ct = (sum(v * l for v, l in zip(rows, lag)) % p for rows in (rows_a, rows_b, rows_c))
    ht = 0
    for c in reversed(h):
        ht = (ht * t + c) % p
    return (at * bt - ct) % p, ht * zt % p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("signed", nargs="?", default=os.path.join(ROOT, "tests", "golden", "falcon_signed.json"),
                    help="JSON with cases of {logn, pk_bytes, msg, sig_bytes} (hex)")
    ap.add_argument("--case", type=int, default=0, help="which of the Falcon-512 cases")
    args = ap.parse_args()
    case = [c for c in json.load(open(args.signed))["cases"] if c["logn"] == 9][args.case]
    p, logn = BN254_FR, 9
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    fft = frw.fft_field_info(p, GENERATOR)
    print("BN254 Fr: two-adicity %d, two-adic root %d" % (fft.two_adicity, fft.two_adic_root))

    eng = frw.WitnessEngine(0)
    sig, pk, hm, st = eng.prepare_inputs(logn, [bytes.fromhex(case["pk_bytes"])], [bytes.fromhex(case["msg"])], [bytes.fromhex(case["sig_bytes"])])
    if st.any():
        raise SystemExit("the encoded inputs were refused: status %s" % st.tolist())
    L = frw.layout(logn)
    d = [torch.from_numpy(a.view(np.int16)).to(dev) for a in (sig, pk, hm)]
    wit = torch.empty((1, L.num_witness, 4), dtype=torch.int64, device=dev)
    inst = torch.empty((1, L.num_instance, 4), dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    eng.witness_ntt_verify_dev(logn, 1, d[0], d[1], d[2], wit, inst, status, eng.field_encoding(p), stream)

    r1cs = eng.r1csf_load(frw.CIRCUIT_NTT, logn, p)
    qap = eng.qapf_create(r1cs, GENERATOR)
    info = eng.qapf_info(qap)
    nc, ni, n = int(info.num_constraints), int(info.num_instance), int(info.domain.size)
    dom = frw.qapf_domain(p, GENERATOR, nc, ni)
    print("the NTT circuit over BN254: C = %d, I = %d, domain 2^%d, %d passes a transform, %.1f MB of workspace a statement"
          % (nc, ni, dom.log_size, info.num_passes, info.workspace_bytes_per_statement / 1e6))
    per = int(info.workspace_bytes_per_statement)
    ws = torch.empty(per, dtype=torch.uint8, device=dev)
    h = torch.empty((1, n, 4), dtype=torch.int64, device=dev)
    num = torch.empty(1, dtype=torch.int32, device=dev)
    eng.qapf_witness_map_dev(qap, 1, wit, inst, h, ws, per, num, stream)

    abc = torch.empty((1, 3, nc, 4), dtype=torch.int64, device=dev)
    need = eng.r1csf_scratch_bytes(r1cs, 1, True)
    scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    eng.r1csf_check_dev(r1cs, 1, wit, inst, cnt, None, abc, scratch, need, stream)
    torch.cuda.synchronize()
    eng.qapf_free(qap)
    eng.r1csf_free(r1cs)
    eng.close()

    rinv = pow(1 << 256, -1, p)
    plain = lambda t: [v * rinv % p for v in to_ints(t)]
    az, bz, cz, hh, inputs = plain(abc[0, 0]), plain(abc[0, 1]), plain(abc[0, 2]), plain(h[0]), plain(inst[0])
    print("the genuine signature: status %d, violated rows: %d, h[n - 1] = %d" % (status.tolist()[0], num.tolist()[0], hh[n - 1]))
    ok = status.tolist() == [0] and num.tolist() == [0] and cnt.tolist() == [0] and hh[n - 1] == 0
    rng = random.Random(254)
    for _ in range(2):
        t = rng.randrange(2, p)
        lhs, rhs = identity_sides(p, dom, az + inputs, bz, cz, hh, t)
        print("A(t) B(t) - C(t) %s h(t) (t^n - 1) at t = %d..." % ("==" if lhs == rhs else "!=", t >> 200))
        ok = ok and lhs == rhs
    if not ok:
        raise SystemExit("expected 0 violated rows and the identity at both points")


if __name__ == "__main__":
    main()
