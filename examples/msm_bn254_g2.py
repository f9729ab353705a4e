#!/usr/bin/env python3
"""The G2 sum of a Groth16 prover over BN254 on the device: frw_curve2_* and frw_msmf2_*.

    python examples/msm_bn254_g2.py

BN254's G2 is the curve y^2 = x^3 + 3 / (9 + u) over Fq2 = Fq[u] / (u^2 + 1), described to the library at run time as
{q, r, nonresidue = q - 1, b'}.  A generator is derived here -- the smallest x = (k, 0) with x^3 + b' a square, times the twist's cofactor
2 q - r, by frw_curve2_scalar_mul -- and a toy "key" b_g2_query[i] = t_i G for t_i drawn here.  A witness z of n values below r lies on
the device in ark-ff's Montgomery form; frw_msmf2_dev returns sum z_i b_g2_query[i], the witness part of a proof's B, and the host's
double-and-add gives (sum z_i t_i mod r) G to compare with.

Exit status 0: the two are equal.
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


def limbs(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint64).reshape(-1, 4).copy()


def mul2(q, a, b):
    """(a0 + a1 u)(b0 + b1 u), u^2 = -1"""
    return ((a[0] * b[0] - a[1] * b[1]) % q, (a[0] * b[1] + a[1] * b[0]) % q)


def sqrt2(q, a):
    """a square root in Fq[u] / (u^2 + 1) for q = 3 mod 4 (the complex method), or None"""
    a0, a1 = a
    root = lambda v: pow(v, (q + 1) // 4, q)
    if a1 == 0:
        s = root(a0)
        if s * s % q == a0:
            return (s, 0)
        s = root(-a0 % q)
        return (0, s) if s * s % q == -a0 % q else None
    n = (a0 * a0 + a1 * a1) % q
    s = root(n)
    if s * s % q != n:
        return None
    for t in ((a0 + s) * pow(2, -1, q) % q, (a0 - s) * pow(2, -1, q) % q):
        x0 = root(t)
        if x0 and x0 * x0 % q == t:
            return (x0, a1 * pow(2 * x0, -1, q) % q)
    return None


def main():
    r, q = BN254_FR, BN254_FQ
    n = 1 << 10
    dev = torch.device("cuda:0")
    mont = lambda v, m: v * (1 << 256) % m
    i82 = pow(82, -1, q)
    b = (27 * i82 % q, -3 * i82 % q)                               # 3 / (9 + u) = 3 (9 - u) / 82
    curve = (q, r, q - 1, b)
    info = frw.curve2_info(*curve)
    print("BN254 G2: q of %d bits, r of %d bits, u^2 = -1 recognised: %s" % (info.base_bits, info.scalar_bits, info.nonresidue_is_minus_one))

    k = 1
    while True:
        x = (k, 0)
        rhs = mul2(q, mul2(q, x, x), x)
        y = sqrt2(q, ((rhs[0] + b[0]) % q, (rhs[1] + b[1]) % q))
        if y is not None:
            break
        k += 1
    point = limbs([mont(v, q) for v in x + y]).reshape(1, 16)
    assert frw.curve2_check_points(*curve, point) == -1
    g = frw.curve2_scalar_mul(*curve, point, limbs([2 * q - r]))    # into the subgroup of order r
    assert g.any() and not frw.curve2_scalar_mul(*curve, g, limbs([r])).any()
    print("generator: x = (%d, 0) cleared of the cofactor 2 q - r; r G is the point at infinity" % k)

    rng = random.Random(254)
    t = [rng.randrange(1, r) for _ in range(n)]
    query = frw.curve2_scalar_mul(*curve, np.repeat(g, n, axis=0), limbs(t))
    z = [rng.randrange(r) for _ in range(n)]
    d_z = torch.from_numpy(limbs([mont(v, r) for v in z]).view(np.int64).reshape(1, n, 4)).to(dev)

    eng = frw.WitnessEngine(0)
    msm = eng.msmf2_load(*curve, query)
    mi = eng.msmf2_info(msm)
    print("b_g2_query: %d points, %d windows of %d bits, %.1f MB of workspace a statement"
          % (mi.num_points, mi.num_windows, mi.window_bits, mi.workspace_bytes_per_statement / 1e6))
    size = eng.msmf2_workspace_bytes(msm, 1)
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    out = torch.empty((1, 16), dtype=torch.int64, device=dev)
    eng.msmf2_dev(msm, 1, d_z, n, n, True, out, ws, size, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    eng.msmf2_free(msm)
    eng.close()

    want = frw.curve2_scalar_mul(*curve, g, limbs([sum(a * c for a, c in zip(z, t)) % r]))
    got = out.cpu().numpy().view(np.uint64)
    ok = np.array_equal(got, want) and got.any()
    print("sum z_i b_g2_query[i] %s (sum z_i t_i) G" % ("==" if ok else "!="))
    if not ok:
        raise SystemExit("the device's sum differs from frw_curve2_scalar_mul's")


if __name__ == "__main__":
    main()
