"""Curves y^2 = x^3 + b' over Fq2 = Fq[u] / (u^2 - beta) in Python integers, for the tests of frw_curve2_* and frw_msmf2_*
(tests/test_curve2_host.py, tests/test_gpu_msm_field2.py): Fq2, affine addition, scalar multiplication, ark-ff's Montgomery packing
(x.c0, x.c1, y.c0, y.c1), and the two curves the tests run over.  An element of Fq2 is (c0, c1); a point is (x, y) or None for the point
at infinity.

* bn254_g2: BN254's twist, beta = -1, b' = 3 / (9 + u).  Its generator is DERIVED here: the smallest x = (k, 0), k = 1, 2, ..., for which
  x^3 + b' is a square (q = 3 mod 4: the complex method), times the twist's cofactor 2 q - r.  Checked at import: on the curve, not
  infinity, r G = infinity.  Sums over a progression are then ONE multiple of G.
* pallas_ext: Fq2 over Pallas' base field with beta = 5 (its multiplicative generator, so a non-residue; q = 1 mod 4, so -1 would not
  do), b' := y^2 - x^3 for a fixed point (x, y).  The group's order is unknown: `order` is None and expected sums use unreduced integer
  multiples.  The only cover of beta != -1."""
from collections import namedtuple

import numpy as np

import curve_reference as R1
import field_cases as F

Curve2 = namedtuple("Curve2", "name q r beta b g order")


def f2_add(c, a, b):
    return ((a[0] + b[0]) % c.q, (a[1] + b[1]) % c.q)


def f2_sub(c, a, b):
    return ((a[0] - b[0]) % c.q, (a[1] - b[1]) % c.q)


def f2_mul(c, a, b):
    return ((a[0] * b[0] + c.beta * a[1] * b[1]) % c.q, (a[0] * b[1] + a[1] * b[0]) % c.q)


def f2_inv(c, a):
    n = pow((a[0] * a[0] - c.beta * a[1] * a[1]) % c.q, -1, c.q)
    return (a[0] * n % c.q, -a[1] * n % c.q)


def f2_scale(c, k, a):
    return (k * a[0] % c.q, k * a[1] % c.q)


def on_curve(c, p):
    if p is None:
        return True
    x, y = p
    if not all(0 <= v < c.q for v in x + y):
        return False
    return f2_mul(c, y, y) == f2_add(c, f2_mul(c, f2_mul(c, x, x), x), c.b)


def neg(c, p):
    return None if p is None else (p[0], (-p[1][0] % c.q, -p[1][1] % c.q))


def add(c, p, s):
    if p is None:
        return s
    if s is None:
        return p
    if p[0] == s[0]:
        if f2_add(c, p[1], s[1]) == (0, 0):
            return None
        lam = f2_mul(c, f2_scale(c, 3, f2_mul(c, p[0], p[0])), f2_inv(c, f2_scale(c, 2, p[1])))
    else:
        lam = f2_mul(c, f2_sub(c, s[1], p[1]), f2_inv(c, f2_sub(c, s[0], p[0])))
    x = f2_sub(c, f2_sub(c, f2_mul(c, lam, lam), p[0]), s[0])
    return (x, f2_sub(c, f2_mul(c, lam, f2_sub(c, p[0], x)), p[1]))


def mul(c, k, p):
    """k p for any integer k >= 0: double-and-add, no reduction of k"""
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = add(c, acc, acc)
        if bit == "1":
            acc = add(c, acc, p)
    return acc


def pack(c, pts):
    """points -> uint64[n, 16]: x.c0, x.c1, y.c0, y.c1, four little-endian limbs of v 2^256 mod q each; infinity all zero"""
    out = np.zeros((len(pts), 16), dtype=np.uint64)
    for i, p in enumerate(pts):
        if p is not None:
            for j, v in enumerate(p[0] + p[1]):
                out[i, 4 * j:4 * j + 4] = F.limbs4(F.mont(v, c.q))
    return out


def unpack(c, arr):
    inv = pow(1 << 256, -1, c.q)
    out = []
    for row in np.asarray(arr, dtype=np.uint64).reshape(-1, 16).tolist():
        v = [sum(w << (64 * i) for i, w in enumerate(row[4 * j:4 * j + 4])) for j in range(4)]
        out.append(None if not any(v) else ((v[0] * inv % c.q, v[1] * inv % c.q), (v[2] * inv % c.q, v[3] * inv % c.q)))
    return out


scalars = R1.scalars


def progression(c, n, s0, d):
    """P_i = (s0 + i d) G for i < n, one affine addition each"""
    p, step, out = mul(c, s0, c.g), mul(c, d, c.g), []
    for _ in range(n):
        out.append(p)
        p = add(c, p, step)
    return out


def progression_sum(c, ks, s0, d):
    """sum k_i P_i over progression(c, len(ks), s0, d) as ONE multiple of G (reduced by the group's order where it is known)"""
    total = sum(k * (s0 + i * d) for i, k in enumerate(ks))
    return mul(c, total % c.order if c.order else total, c.g)


def _sqrt_complex(q, a):
    """a square root of a in Fq[u] / (u^2 + 1), q = 3 mod 4, or None"""
    a0, a1 = a
    if a1 == 0:
        s = pow(a0, (q + 1) // 4, q)
        if s * s % q == a0:
            return (s, 0)
        s = pow(-a0 % q, (q + 1) // 4, q)                       # a0 is no square: -a0 is, and (s u)^2 = -s^2 = a0
        return (0, s) if s * s % q == -a0 % q else None
    n = (a0 * a0 + a1 * a1) % q
    s = pow(n, (q + 1) // 4, q)
    if s * s % q != n:
        return None
    half = pow(2, -1, q)
    for t in ((a0 + s) * half % q, (a0 - s) * half % q):
        x0 = pow(t, (q + 1) // 4, q)
        if x0 and x0 * x0 % q == t:
            x1 = a1 * pow(2 * x0, -1, q) % q
            return (x0, x1)
    return None


def _bn254_g2():
    q, r = R1.BN254.q, R1.BN254.r
    assert q % 4 == 3
    i82 = pow(82, -1, q)
    proto = Curve2("bn254_g2", q, r, q - 1, (27 * i82 % q, -3 * i82 % q), None, r)        # 3 / (9 + u) = 3 (9 - u) / 82
    assert f2_mul(proto, proto.b, (9, 1)) == (3, 0)
    k = 1
    while True:
        x = (k, 0)
        y = _sqrt_complex(q, f2_add(proto, f2_mul(proto, f2_mul(proto, x, x), x), proto.b))
        if y is not None:
            break
        k += 1
    assert on_curve(proto, (x, y))
    g = mul(proto, 2 * q - r, (x, y))
    c = proto._replace(g=g)
    assert g is not None and on_curve(c, g) and mul(c, r, g) is None
    return c


def _pallas_ext():
    q = F.PALLAS
    assert q % 4 == 1 and pow(5, (q - 1) // 2, q) == q - 1                              # 5 is a non-residue
    proto = Curve2("pallas_ext", q, R1.PALLAS_R, 5, (0, 0), None, None)
    x, y = (1, 2), (3, 4)
    b = f2_sub(proto, f2_mul(proto, y, y), f2_mul(proto, f2_mul(proto, x, x), x))
    c = proto._replace(b=b, g=(x, y))
    assert b != (0, 0) and on_curve(c, c.g)
    return c


BN254_G2 = _bn254_g2()
PALLAS_EXT = _pallas_ext()
CURVES = {c.name: c for c in (BN254_G2, PALLAS_EXT)}
