"""ark-serialize's wire format for BLS12-381 points, proofs and verifying keys (ark-serialize / ark-ec 0.3), restated in Python integers
for the tests of the library's codec -- independent of the C++: roots by pow(), the Fq2 root by the "complex method" for q = 3 (mod 4)
(the library goes through the norm), points as oracle/bls12_381.py keeps them ((x, y) tuples, None = infinity; Fq2 values (c0, c1)).

  Fq    48 bytes little-endian, the canonical integer;  Fq2: c0 then c1
  flags in the top two bits of the last byte: 0x80 "y is the greater of y, -y", 0x40 infinity
  compressed: x with flags;  uncompressed: x, then y with the infinity flag only
  proof: A | B | C;  key: alpha_g1 | beta_g2 | gamma_g2 | delta_g2 | le64(n) | gamma_abc_g1[n]
Strict: one encoding per point (both flags, infinity with a non-zero coordinate, bit 7 in an uncompressed point are malformed)."""
from oracle import bls12_381 as E

Q = E.Q
GREATER, INFINITY = 0x80, 0x40


class Malformed(ValueError):
    pass


def fq_greater(y):
    return y > (Q - y) % Q


def fq2_greater(y):
    """ark orders Fq2 by c1 first, then c0"""
    n = ((-y[0]) % Q, (-y[1]) % Q)
    return y[1] > n[1] if y[1] != n[1] else y[0] > n[0]


def _fq(v, flags=0):
    b = bytearray(v.to_bytes(48, "little"))
    b[47] |= flags
    return bytes(b)


def _fq2(v, flags=0):
    return _fq(v[0]) + _fq(v[1], flags)


def g1_encode(p, compressed=True):
    if p is None:
        return _fq(0, INFINITY) if compressed else _fq(0) + _fq(0, INFINITY)
    if compressed:
        return _fq(p[0], GREATER if fq_greater(p[1]) else 0)
    return _fq(p[0]) + _fq(p[1])


def g2_encode(p, compressed=True):
    if p is None:
        return _fq2((0, 0), INFINITY) if compressed else _fq2((0, 0)) + _fq2((0, 0), INFINITY)
    if compressed:
        return _fq2(p[0], GREATER if fq2_greater(p[1]) else 0)
    return _fq2(p[0]) + _fq2(p[1])


def fq_sqrt(a):
    r = pow(a, (Q + 1) // 4, Q)
    return r if r * r % Q == a % Q else None


def _f2_pow(a, e):
    acc = (1, 0)
    while e:
        if e & 1:
            acc = E.f2_mul(acc, a)
        a = E.f2_mul(a, a)
        e >>= 1
    return acc


def fq2_sqrt(a):
    """Adj, Rodriguez-Henriquez, "Square root computation over even extension fields", algorithm 9 (q = 3 mod 4)"""
    a = (a[0] % Q, a[1] % Q)
    if a == (0, 0):
        return (0, 0)
    a1 = _f2_pow(a, (Q - 3) // 4)
    alpha = E.f2_mul(a1, E.f2_mul(a1, a))
    a0 = E.f2_mul((alpha[0], (-alpha[1]) % Q), alpha)
    if a0 == (Q - 1, 0):
        return None
    x0 = E.f2_mul(a1, a)
    if alpha == (Q - 1, 0):
        x = E.f2_mul((0, 1), x0)
    else:
        x = E.f2_mul(_f2_pow(E.f2_add((1, 0), alpha), (Q - 1) // 2), x0)
    return x if E.f2_mul(x, x) == a else None


def _take_fq(b, flagged):
    """48 bytes -> (value, flags); flags are masked off before the range test"""
    flags = b[47] & 0xC0 if flagged else 0
    v = int.from_bytes(b[:47] + bytes([b[47] & 0x3F if flagged else b[47]]), "little")
    if v >= Q:
        raise Malformed("a field element >= q")
    return v, flags


def g1_decode(b, compressed=True):
    b = bytes(b)
    if compressed:
        x, flags = _take_fq(b[:48], True)
        y = None
    else:
        x, _ = _take_fq(b[:48], False)
        y, flags = _take_fq(b[48:96], True)
        if flags & GREATER:
            raise Malformed("bit 7 in an uncompressed point")
    if flags == GREATER | INFINITY:
        raise Malformed("both flags")
    if flags & INFINITY:
        if x or y:
            raise Malformed("infinity with a non-zero coordinate")
        return None
    rhs = (x * x * x + 4) % Q
    if compressed:
        y = fq_sqrt(rhs)
        if y is None:
            raise Malformed("no y for this x")
        if fq_greater(y) != bool(flags & GREATER):
            y = (-y) % Q
    elif y * y % Q != rhs:
        raise Malformed("off the curve")
    return (x, y)


def g2_decode(b, compressed=True):
    b = bytes(b)
    x0, _ = _take_fq(b[:48], False)
    if compressed:
        x1, flags = _take_fq(b[48:96], True)
        y = None
    else:
        x1, _ = _take_fq(b[48:96], False)
        y0, _ = _take_fq(b[96:144], False)
        y1, flags = _take_fq(b[144:192], True)
        y = (y0, y1)
        if flags & GREATER:
            raise Malformed("bit 7 in an uncompressed point")
    if flags == GREATER | INFINITY:
        raise Malformed("both flags")
    x = (x0, x1)
    if flags & INFINITY:
        if x != (0, 0) or (y is not None and y != (0, 0)):
            raise Malformed("infinity with a non-zero coordinate")
        return None
    rhs = E.f2_add(E.f2_mul(E.f2_mul(x, x), x), (4, 4))
    if compressed:
        y = fq2_sqrt(rhs)
        if y is None:
            raise Malformed("no y for this x")
        if fq2_greater(y) != bool(flags & GREATER):
            y = ((-y[0]) % Q, (-y[1]) % Q)
    elif E.f2_mul(y, y) != rhs:
        raise Malformed("off the curve")
    return (x, y)


def g1_len(compressed):
    return 48 if compressed else 96


def g2_len(compressed):
    return 96 if compressed else 192


def proof_encode(proof, compressed=True):
    return g1_encode(proof[0], compressed) + g2_encode(proof[1], compressed) + g1_encode(proof[2], compressed)


def proof_decode(b, compressed=True):
    n1, n2 = g1_len(compressed), g2_len(compressed)
    if len(b) != 2 * n1 + n2:
        raise Malformed("length")
    return (g1_decode(b[:n1], compressed), g2_decode(b[n1:n1 + n2], compressed), g1_decode(b[n1 + n2:], compressed))


def vk_encode(vk, compressed=True):
    """vk: the dict of points tests/test_pairing_host.py::make_statement returns"""
    out = g1_encode(vk["alpha_g1"], compressed)
    for k in ("beta_g2", "gamma_g2", "delta_g2"):
        out += g2_encode(vk[k], compressed)
    out += len(vk["gamma_abc_g1"]).to_bytes(8, "little")
    for p in vk["gamma_abc_g1"]:
        out += g1_encode(p, compressed)
    return out
