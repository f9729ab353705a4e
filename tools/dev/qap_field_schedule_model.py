"""Exact-integer model of the pass schedule of frw_qap_field.hip (the rule at the head of falcon-r1cs_amd/csrc/frw_qap_field.h): the
digits, the tiles a workgroup takes (which positions, by the same bit insertions as the kernel), the twists, the digit-reversed order and
the write of h through it -- against the plain witness map of tests/qap_field_reference.py over a 31-bit field.  A pass here is what a
workgroup does: gather its tile, a plain 2^T-point transform per column, one multiplication per element, store.

    python tools/dev/qap_field_schedule_model.py            # the device's constants, L = 1 .. 14, and smaller ones that reach three passes
"""
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import qap_field_reference as ref

P, G = 15 * 2**27 + 1, 31


def schedule(L, lds_log=12, max_digit=8):
    m = 1 if L <= lds_log else (L + max_digit - 1) // max_digit
    T = [L // m + (1 if i < L % m else 0) for i in range(m)]
    S = [sum(T[i + 1:]) for i in range(m)]
    return T, S


def digit_reverse(T, S, pos):
    index, sh = 0, 0
    for t, s in zip(T, S):
        index |= ((pos >> s) & ((1 << t) - 1)) << sh
        sh += t
    return index


def insert(x, shift, width):
    return ((x >> shift) << (shift + width)) | (x & ((1 << shift) - 1))


def tile_positions(L, T, c, t_shift, u_shift):
    """what the kernel computes: for every tile w, the positions of its elements (t, u)"""
    lo, hi = sorted([(t_shift, T), (u_shift, c)])
    for w in range(1 << (L - T - c)):
        base = insert(insert(w, *lo), *hi)
        yield [[base | t << t_shift | u << u_shift for u in range(1 << c)] for t in range(1 << T)]


def dft(vals, root):
    """sum_j vals[j] root^(j k) at k: natural in, natural out"""
    n = len(vals)
    if n == 1:
        return list(vals)
    even, odd = dft(vals[0::2], root * root % P), dft(vals[1::2], root * root % P)
    out, x = [0] * n, 1
    for k in range(n // 2):
        t = x * odd[k] % P
        out[k], out[k + n // 2] = (even[k] + t) % P, (even[k] - t) % P
        x = x * root % P
    return out


def run_pass(L, src, T, c, t_shift, u_shift, root, post=None, post_mask=0, scatter=None):
    """src: position -> value; returns the array after the pass.  post: table indexed by (position, or the scattered index) & post_mask"""
    n = 1 << L
    out = [None] * n
    rho = pow(root, n >> T, P)
    for tile in tile_positions(L, T, c, t_shift, u_shift):
        for u in range(1 << c):
            col = dft([src(tile[t][u]) for t in range(1 << T)], rho)
            for t in range(1 << T):
                pos = tile[t][u]
                dst = scatter(pos) if scatter else pos
                v = col[t]
                if post is not None:
                    v = v * post[dst & post_mask] % P
                assert out[dst] is None
                out[dst] = v
    assert None not in out
    return out


def twist_table(L, T, S, i, root):
    wb = pow(root, 1 << (L - S[i] - T[i]), P)
    return [pow(wb, (x >> S[i]) * (x & ((1 << S[i]) - 1)), P) for x in range(1 << (S[i] + T[i]))]


def placement(L, T, S, i, c, last_of_map=False):
    """(t_shift, u_shift) of pass i"""
    if len(T) == 1:
        return 0, L
    if S[i] == 0:
        return 0, (S[0] if last_of_map else T[i])
    assert S[i] >= c
    return S[i], 0


def witness_map(L, az, bz, cz, inputs, lds_log=12, max_digit=8, cols=3):
    n = 1 << L
    T, S = schedule(L, lds_log, max_digit)
    m = len(T)
    c = 0 if m == 1 else cols
    assert all(t + c <= max(lds_log, max_digit + cols) for t in T) and (m == 1 or (T[-1] >= c and T[0] >= c))
    d = ref.Domain(P, G, n)
    w, wi = d.group_gen, d.group_gen_inv
    rev = lambda pos: digit_reverse(T, S, pos)
    scale_in = [None] * n
    for pos in range(n):
        scale_in[pos] = pow(G, rev(pos), P) * d.size_inv % P
    scale_out = [pow(d.generator_inv, k, P) * d.size_inv * d.vanishing_inv % P for k in range(n)]
    nc = len(az)
    rows = [list(az) + list(inputs), list(bz), list(cz)]
    work = []
    for which in range(3):
        arr = lambda pos, r=rows[which]: r[pos] if pos < len(r) else 0       # A z ++ instance ++ 0, read on the fly
        for i in range(m):                                                     # F(w^-1), then x g^rev(pos) / n
            post, mask = (twist_table(L, T, S, i, wi), (1 << (S[i] + T[i])) - 1) if i < m - 1 else (scale_in, n - 1)
            a = run_pass(L, arr, T[i], c, *placement(L, T, S, i, c), wi, post, mask)
            arr = lambda pos, a=a: a[pos]
        for i in range(m - 1, -1, -1):                                         # G(w)
            post, mask = (twist_table(L, T, S, i - 1, w), (1 << (S[i - 1] + T[i - 1])) - 1) if i > 0 else (None, 0)
            a = run_pass(L, arr, T[i], c, *placement(L, T, S, i, c), w, post, mask)
            arr = lambda pos, a=a: a[pos]
        work.append(a)
    arr = lambda pos: (work[0][pos] * work[1][pos] - work[2][pos]) % P          # fused into the first pass
    for i in range(m):
        if i < m - 1:
            a = run_pass(L, arr, T[i], c, *placement(L, T, S, i, c), wi, twist_table(L, T, S, i, wi), (1 << (S[i] + T[i])) - 1)
        else:
            a = run_pass(L, arr, T[i], c, *placement(L, T, S, i, c, True), wi, scale_out, n - 1, scatter=rev)
        arr = lambda pos, a=a: a[pos]
    return a, nc


def check(L, **kw):
    rng = random.Random(L)
    n = 1 << L
    for nc in sorted({n - 2, n // 2 - 1} - {0, -1}) or [1]:
        ni = 2 if nc + 2 <= n else 1
        az, bz, cz = ([rng.randrange(P) for _ in range(nc)] for _ in range(3))
        inputs = [rng.randrange(P) for _ in range(ni)]
        got, _ = witness_map(L, az, bz, cz, inputs, **kw)
        assert got == ref.witness_map(P, G, az, bz, cz, inputs), (L, nc, kw)


def main():
    for L in range(1, 15):
        check(L)
        print("L = %2d  digits %s: equal" % (L, schedule(L)[0]))
    for L in range(4, 11):                                   # the same rule with small constants: two and three passes at sizes a plain DFT affords
        for max_digit, cols in ((3, 1), (4, 2), (3, 0)):
            if L > max_digit and min(schedule(L, max_digit, max_digit)[0]) >= cols:
                check(L, lds_log=max_digit, max_digit=max_digit, cols=cols)
                print("L = %2d  digits %s, %d columns: equal" % (L, schedule(L, max_digit, max_digit)[0], 1 << cols))


if __name__ == "__main__":
    main()
