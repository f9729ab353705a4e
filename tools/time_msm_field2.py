"""Time the multi-scalar multiplication over a curve on a run-time Fq2, frw_msmf2_dev, beside two yardsticks already in the tree, in one
process: n = 2^18 - 1 points (--points overrides), uniform scalars below r in Montgomery form, batch 1 and 16, HIP events around five
back-to-back calls after a warm-up --
  frw_msmf2_dev over BN254's G2 (u^2 = -1, b' = 3 / (9 + u); the generator derived here: the smallest x = (k, 0) on the curve, times 2 q - r),
  frw_msmf_dev over BN254 G1 at the same n: the G2 / G1 ratio is to be read against the 28 : 10 count of field products in the two mixed
  additions,
  frw_msm_g2_dev on a DENSE BARE BLS12-381 handle (frw_msm_g2_load_bare, narrow = 0): the same schedule with the curve compiled in
-- and each result of the new call is compared with the one multiple of G it must be (the bases are a progression (s0 + i d) G).
A record, judged against nothing.

Writes the figures to --out (default profiles/msm_field2.txt).
usage: python tools/time_msm_field2.py [--points N] [--launches 5] [--out PATH]
       rocprofv3 --kernel-trace --stats --output-format csv -- python tools/time_msm_field2.py --trace BATCH
           (three calls over BN254's G2 at that batch and nothing else: the per-kernel split, profiles/msm_field2_kernel_split.txt)"""
import os
import random
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import falcon_r1cs_amd as frw

BN254_FR = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
BN254_FQ = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
BLS12_381_FR = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
S0, D = 0x1234567, 0x89AB
BATCHES = (1, 16)
G2_NAME, G1_NAME, YARD = "BN254 G2", "BN254 G1", "BLS12-381 G2, dense bare handle"


def arg(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


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


def progression(q, width, g, first, step, n):
    """(first + i step) G for i < n as Montgomery limbs uint64[n, 8 width]: affine chord additions in Python integers; width 1 is Fq
    (a coordinate an integer), width 2 is Fq[u] / (u^2 + 1) (a coordinate a pair)"""
    if width == 1:
        fmul = lambda a, b: a * b % q
        finv = lambda a: pow(a, -1, q)
        fsub = lambda a, b: (a - b) % q
        scale = lambda k, a: k * a % q
        flat = lambda a: [a]
    else:
        fmul = lambda a, b: mul2(q, a, b)
        fsub = lambda a, b: ((a[0] - b[0]) % q, (a[1] - b[1]) % q)
        scale = lambda k, a: (k * a[0] % q, k * a[1] % q)
        flat = list

        def finv(a):
            n_ = pow((a[0] * a[0] + a[1] * a[1]) % q, -1, q)
            return (a[0] * n_ % q, -a[1] * n_ % q)

    def add(p, s):
        if p[0] == s[0]:
            lam = fmul(scale(3, fmul(p[0], p[0])), finv(scale(2, p[1])))
        else:
            lam = fmul(fsub(s[1], p[1]), finv(fsub(s[0], p[0])))
        x = fsub(fsub(fmul(lam, lam), p[0]), s[0])
        return (x, fsub(fmul(lam, fsub(p[0], x)), p[1]))

    def mul(k):
        acc = None
        for bit in bin(k)[2:]:
            acc = add(acc, acc) if acc else None
            if bit == "1":
                acc = add(acc, g) if acc else g
        return acc

    p, d, coords = mul(first), mul(step), []
    for _ in range(n):
        coords += [v << 256 for v in flat(p[0]) + flat(p[1])]
        p = add(p, d)
    return limbs([v % q for v in coords]).reshape(n, 8 * width)


def g2_curve_and_generator():
    """-> (the descriptor (q, r, nonresidue, b'), G as Python pairs, G as uint64[1, 16])"""
    q, r = BN254_FQ, BN254_FR
    i82 = pow(82, -1, q)
    b = (27 * i82 % q, -3 * i82 % q)
    curve = (q, r, q - 1, b)
    k = 1
    while True:
        x = (k, 0)
        rhs = mul2(q, mul2(q, x, x), x)
        y = sqrt2(q, ((rhs[0] + b[0]) % q, (rhs[1] + b[1]) % q))
        if y is not None:
            break
        k += 1
    g = frw.curve2_scalar_mul(*curve, limbs([v * (1 << 256) % q for v in x + y]).reshape(1, 16), limbs([2 * q - r]))
    assert g.any() and not frw.curve2_scalar_mul(*curve, g, limbs([r])).any()
    rinv = pow(1 << 256, -1, q)
    v = [int.from_bytes(g[0, 4 * j:4 * j + 4].tobytes(), "little") * rinv % q for j in range(4)]
    return curve, ((v[0], v[1]), (v[2], v[3])), g


def main():
    import torch
    dev = torch.device("cuda:0")
    eng = frw.WitnessEngine(0)
    launches = arg("--launches", 5)
    n = arg("--points", (1 << 18) - 1)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "msm_field2.txt"), str)
    s0 = torch.cuda.current_stream().cuda_stream
    rng = random.Random(18)
    q, r = BN254_FQ, BN254_FR

    def timed(fn):
        fn()                                                     # warm-up
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / launches / 1e3

    def uniform(modulus, batch):
        """-> (integers [batch][n], their Montgomery form on the device)"""
        row = [rng.randrange(modulus) for _ in range(n)]        # (a statement's scalars: the first one's times a unit, as uniform and quicker to make)
        ks = [row] + [[k * c % modulus for k in row] for c in (rng.randrange(2, modulus) for _ in range(batch - 1))]
        return ks, torch.from_numpy(limbs([k * (1 << 256) % modulus for row in ks for k in row]).view(np.int64).reshape(batch, n, 4)).to(dev)

    curve2, g2, g2m = g2_curve_and_generator()
    bases2 = progression(q, 2, g2, S0, D, n)
    trace = arg("--trace", 0)
    if trace:
        h = eng.msmf2_load(*curve2, bases2, frw.MSMF_POINTS_ARE_CHECKED)
        _, d_ks = uniform(r, trace)
        size = eng.msmf2_workspace_bytes(h, trace)
        ws = torch.empty(size, dtype=torch.uint8, device=dev)
        out = torch.empty((trace, 16), dtype=torch.int64, device=dev)
        for _ in range(3):
            eng.msmf2_dev(h, trace, d_ks, n, n, True, out, ws, size, s0)
        torch.cuda.synchronize()
        eng.msmf2_free(h)
        eng.close()
        return

    times, shape = {}, {}
    multiples = lambda ks: limbs([sum(k * (S0 + i * D) for i, k in enumerate(row)) % r for row in ks])
    h = eng.msmf2_load(*curve2, bases2)
    info = eng.msmf2_info(h)
    shape[G2_NAME] = (int(info.window_bits), int(info.num_windows), int(info.workspace_bytes_per_statement))
    for batch in BATCHES:
        ks, d_ks = uniform(r, batch)
        size = eng.msmf2_workspace_bytes(h, batch)
        ws = torch.empty(size, dtype=torch.uint8, device=dev)
        out = torch.empty((batch, 16), dtype=torch.int64, device=dev)
        times[G2_NAME, batch] = timed(lambda: eng.msmf2_dev(h, batch, d_ks, n, n, True, out, ws, size, s0))
        want = frw.curve2_scalar_mul(*curve2, np.repeat(g2m, batch, axis=0), multiples(ks))
        assert np.array_equal(out.cpu().numpy().view(np.uint64), want), "G2, batch %d: the sum is not the multiple of G it must be" % batch
        del ws, d_ks
    eng.msmf2_free(h)

    g1 = (1, 2)
    h = eng.msmf_load(q, r, 3, progression(q, 1, g1, S0, D, n))
    info = eng.msmf_info(h)
    shape[G1_NAME] = (int(info.window_bits), int(info.num_windows), int(info.workspace_bytes_per_statement))
    g1m = np.concatenate([limbs([g1[0] * (1 << 256) % q]), limbs([g1[1] * (1 << 256) % q])], axis=1)
    for batch in BATCHES:
        ks, d_ks = uniform(r, batch)
        size = eng.msmf_workspace_bytes(h, batch)
        ws = torch.empty(size, dtype=torch.uint8, device=dev)
        out = torch.empty((batch, 8), dtype=torch.int64, device=dev)
        times[G1_NAME, batch] = timed(lambda: eng.msmf_dev(h, batch, d_ks, n, n, True, out, ws, size, s0))
        want = frw.curve_scalar_mul(q, r, 3, np.repeat(g1m, batch, axis=0), multiples(ks))
        assert np.array_equal(out.cpu().numpy().view(np.uint64), want), "G1, batch %d: the sum is not the multiple of G it must be" % batch
        del ws, d_ks
    eng.msmf_free(h)

    bases = eng.g2_fixed_base(limbs([rng.randrange(1, BLS12_381_FR) for _ in range(n)]))
    h = eng.msm_g2_load(bases, bare=True)
    per = int(eng.msm_info(h).workspace_bytes_per_signature)
    for batch in BATCHES:
        _, d_ks = uniform(BLS12_381_FR, batch)
        ws = torch.empty(batch * per, dtype=torch.uint8, device=dev)
        out = torch.empty((batch, 24), dtype=torch.int64, device=dev)
        times[YARD, batch] = timed(lambda: eng.msm_g2_dev(h, batch, d_ks, n, True, out, ws, batch * per, s0))
        del ws, d_ks
    eng.msm_free(h)
    eng.close()

    lines = ["# tools/time_msm_field2.py: n = %d points, uniform scalars below r in Montgomery form; HIP events, mean of %d back-to-back calls after a"
             % (n, launches),
             "# warm-up, one process; every frw_msmf2_dev and frw_msmf_dev result equals the multiple of G it must be"]
    for name in (G2_NAME, G1_NAME):
        lines.append("# %s: %d windows of %d bits, %.1f MB of workspace a statement" % (name, shape[name][1], shape[name][0], shape[name][2] / 1e6))
    for name, call in ((G2_NAME, "frw_msmf2_dev"), (G1_NAME, "frw_msmf_dev"), (YARD, "frw_msm_g2_dev")):
        for batch in BATCHES:
            t = times[name, batch]
            lines.append("%-15s %-32s batch %2d  %9.3f ms   %8.3f ms/statement   %7.2f ns/point" % (call + ",", name, batch, t * 1e3, t / batch * 1e3, t / batch / n * 1e9))
    for other in (G1_NAME, YARD):
        for batch in BATCHES:
            lines.append("ratio %s / %-32s batch %2d   %6.2f" % (G2_NAME, other + ",", batch, times[G2_NAME, batch] / times[other, batch]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
