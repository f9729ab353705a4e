"""Short Weierstrass curves y^2 = x^3 + b in Python integers, for the tests of frw_curve_* and frw_msmf_* (tests/test_curve_host.py,
tests/test_gpu_msm_field.py): affine addition, doubling, scalar multiplication, ark-ff's Montgomery packing, and the four curves the
tests run over.  A point is (x, y) or None for the point at infinity."""
from collections import namedtuple

import numpy as np

import field_cases as F

Curve = namedtuple("Curve", "name q r b g")

BN254_Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
PALLAS_R = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001
BN254 = Curve("bn254", BN254_Q, F.BN254, 3, (1, 2))
PALLAS = Curve("pallas", F.PALLAS, PALLAS_R, 5, (F.PALLAS - 1, 2))
VESTA = Curve("vesta", PALLAS_R, F.PALLAS, 5, (PALLAS_R - 1, 2))
GRUMPKIN = Curve("grumpkin", F.BN254, BN254_Q, F.BN254 - 17, (1, 0x2CF135E7506A45D632D270D45F1181294833FC48D823F272C))
CURVES = {c.name: c for c in (BN254, PALLAS, VESTA, GRUMPKIN)}


def on_curve(c, p):
    return p is None or (0 <= p[0] < c.q and 0 <= p[1] < c.q and (p[1] * p[1] - p[0] ** 3 - c.b) % c.q == 0)


def neg(c, p):
    return None if p is None else (p[0], -p[1] % c.q)


def add(c, p, s):
    if p is None:
        return s
    if s is None:
        return p
    q = c.q
    if p[0] == s[0]:
        if (p[1] + s[1]) % q == 0:
            return None
        lam = 3 * p[0] * p[0] * pow(2 * p[1], -1, q) % q
    else:
        lam = (s[1] - p[1]) * pow(s[0] - p[0], -1, q) % q
    x = (lam * lam - p[0] - s[0]) % q
    return (x, (lam * (p[0] - x) - p[1]) % q)


def mul(c, k, p):
    """k p for any integer k >= 0: double-and-add, no reduction of k"""
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = add(c, acc, acc)
        if bit == "1":
            acc = add(c, acc, p)
    return acc


def pack(c, pts):
    """points -> uint64[n, 8]: x then y, four little-endian limbs of v 2^256 mod q each; infinity all zero"""
    out = np.zeros((len(pts), 8), dtype=np.uint64)
    for i, p in enumerate(pts):
        if p is not None:
            out[i, :4] = F.limbs4(F.mont(p[0], c.q))
            out[i, 4:] = F.limbs4(F.mont(p[1], c.q))
    return out


def unpack(c, arr):
    inv = pow(1 << 256, -1, c.q)
    out = []
    for row in np.asarray(arr, dtype=np.uint64).reshape(-1, 8).tolist():
        x = sum(v << (64 * i) for i, v in enumerate(row[:4]))
        y = sum(v << (64 * i) for i, v in enumerate(row[4:]))
        out.append(None if x == 0 and y == 0 else (x * inv % c.q, y * inv % c.q))
    return out


def scalars(ks, r=None):
    """integers -> uint64[n, 4]; with r, ark-ff's Montgomery form k 2^256 mod r"""
    return np.array([F.limbs4(k if r is None else F.mont(k, r)) for k in ks], dtype=np.uint64).reshape(-1, 4)


def progression(c, n, s0, d):
    """P_i = (s0 + i d) G for i < n, one affine addition each"""
    p, step, out = mul(c, s0 % c.r, c.g), mul(c, d % c.r, c.g), []
    for _ in range(n):
        out.append(p)
        p = add(c, p, step)
    return out


def progression_sum(c, ks, s0, d):
    """sum k_i P_i over progression(c, len(ks), s0, d) as ONE multiple of G"""
    return mul(c, sum(k * (s0 + i * d) for i, k in enumerate(ks)) % c.r, c.g)
