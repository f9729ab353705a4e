#!/usr/bin/env python3
"""Groth16's `h_acc` over BN254, on the device from the witness to the group element: frw_r1csf_* -> frw_qapf_* -> frw_msmf_*.

    python examples/msm_bn254.py

A small system over BN254's Fr -- a chain of squarings w_(i+1) = w_i^2 whose last value is public, on a domain of 2^10 points -- and a
toy "key": h_query[i] = tau^i G on BN254 G1 (y^2 = x^3 + 3, G = (1, 2)) for a tau drawn here, made on the host with
frw_curve_scalar_mul.  frw_qapf_witness_map_dev writes h, the coefficients of (A(X) B(X) - C(X)) / (X^n - 1), in ark-ff's Montgomery
form; frw_msmf_dev reads them where they lie (scalar_stride = n, num_scalars = n - 1, which is what ark-groth16 sums) and returns
h_acc = sum h_i h_query[i].  Then h(tau) is evaluated in Python integers from a copy of h and h_acc is compared with h(tau) G.

Exit status 0: 0 violated rows and h_acc == h(tau) G.
"""
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import falcon_r1cs_amd as frw

BN254_FR = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
BN254_FQ = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
B, G = 3, (1, 2)
GENERATOR = 5           # ark-bn254's FrParameters::GENERATOR


def limbs(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint64).reshape(-1, 4).copy()


def to_ints(a):
    return [int.from_bytes(r.tobytes(), "little") for r in np.ascontiguousarray(a).view(np.uint64).reshape(-1, 4)]


def main():
    p, q = BN254_FR, BN254_FQ
    n, ni = 1 << 10, 2
    nc = n - ni
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    mont = lambda v, m: v * (1 << 256) % m
    curve = frw.curve_info(q, p, B)
    print("BN254 G1: q of %d bits, r of %d bits, b = %d" % (curve.base_bits, curve.scalar_bits, curve.b))

    # the system: rows i < C: w_i w_i = w_(i+1); column 0 the constant one, column 1 the public last value, 2 + k witness k
    ptr = np.arange(nc + 1, dtype=np.uint64)
    ab = np.arange(ni, ni + nc, dtype=np.uint32)
    c = ab + 1
    c[-1] = 1
    one = np.tile(limbs([1]), (nc, 1))
    w = [0xC0FFEE]
    for _ in range(nc):
        w.append(w[-1] * w[-1] % p)
    inst = torch.from_numpy(limbs([mont(v, p) for v in (1, w[nc])]).view(np.int64).reshape(1, ni, 4)).to(dev)
    wit = torch.from_numpy(limbs([mont(v, p) for v in w[:nc]]).view(np.int64).reshape(1, nc, 4)).to(dev)

    # the toy key: h_query[i] = tau^i G
    tau = random.Random(254).randrange(2, p)
    g = np.concatenate([limbs([mont(G[0], q)]), limbs([mont(G[1], q)])], axis=1)
    h_query = frw.curve_scalar_mul(q, p, B, np.repeat(g, n, axis=0), limbs([pow(tau, i, p) for i in range(n)]))
    assert frw.curve_check_points(q, p, B, h_query) == -1

    eng = frw.WitnessEngine(0)
    r1cs = eng.r1csf_load_csr(p, ni, nc, [(ptr, ab, one), (ptr, ab, one), (ptr, c, one)])
    qap = eng.qapf_create(r1cs, GENERATOR)
    msm = eng.msmf_load(q, p, B, h_query)
    qi, mi = eng.qapf_info(qap), eng.msmf_info(msm)
    assert int(qi.domain.size) == n
    print("h_query: %d points, %d windows of %d bits, %.1f MB of workspace a statement"
          % (mi.num_points, mi.num_windows, mi.window_bits, mi.workspace_bytes_per_statement / 1e6))
    per = int(qi.workspace_bytes_per_statement)
    ws = torch.empty(per, dtype=torch.uint8, device=dev)
    h = torch.empty((1, n, 4), dtype=torch.int64, device=dev)
    num = torch.empty(1, dtype=torch.int32, device=dev)
    size = eng.msmf_workspace_bytes(msm, 1)
    mws = torch.empty(size, dtype=torch.uint8, device=dev)
    h_acc = torch.empty((1, 8), dtype=torch.int64, device=dev)
    eng.qapf_witness_map_dev(qap, 1, wit, inst, h, ws, per, num, stream)
    eng.msmf_dev(msm, 1, h, n, n - 1, True, h_acc, mws, size, stream)          # h never leaves the device on its way here
    torch.cuda.synchronize()
    eng.msmf_free(msm)
    eng.qapf_free(qap)
    eng.r1csf_free(r1cs)
    eng.close()

    rinv = pow(1 << 256, -1, p)
    hh = [v * rinv % p for v in to_ints(h[0].cpu().numpy())]
    h_tau = 0
    for v in reversed(hh):
        h_tau = (h_tau * tau + v) % p
    want = frw.curve_scalar_mul(q, p, B, g, limbs([h_tau]))
    got = h_acc.cpu().numpy().view(np.uint64)
    print("violated rows: %d, h[n - 1] = %d" % (num.tolist()[0], hh[n - 1]))
    ok = num.tolist() == [0] and hh[n - 1] == 0 and np.array_equal(got, want)
    print("h_acc %s h(tau) G" % ("==" if ok else "!="))
    if not ok:
        raise SystemExit("expected 0 violated rows and h_acc == h(tau) G")


if __name__ == "__main__":
    main()
