"""Time the multi-scalar multiplication over a run-time curve, frw_msmf_dev, beside the yardstick already in the tree, in one process:
n = 2^18 - 1 points (--points overrides), uniform scalars below r in Montgomery form, batch 1 and 16, HIP events around five back-to-back
calls after a warm-up --
  frw_msmf_dev over BN254 G1,
  frw_msmf_dev over Pallas,
  frw_msm_g1_dev on a DENSE BARE BLS12-381 handle (frw_msm_g1_load_bare, narrow = 0): the same schedule -- no window tables, window
  sums joined by Horner's rule -- with the curve compiled in
-- and each result of the new call is compared with the one multiple of G it must be (the bases are a progression (s0 + i d) G).
A record, judged against nothing.

Writes the figures to --out (default profiles/msm_field.txt).
usage: python tools/time_msm_field.py [--points N] [--launches 5] [--out PATH]
       rocprofv3 --kernel-trace --stats --output-format csv -- python tools/time_msm_field.py --trace BATCH
           (three calls over BN254 G1 at that batch and nothing else: the per-kernel split, profiles/msm_field_kernel_split.txt)"""
import os
import random
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import falcon_r1cs_amd as frw

BN254_FR = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
BN254_FQ = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
PALLAS_FQ = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001
PALLAS_FR = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001
BLS12_381_FR = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
CURVES = (("BN254 G1", BN254_FQ, BN254_FR, 3, (1, 2)), ("Pallas", PALLAS_FQ, PALLAS_FR, 5, (PALLAS_FQ - 1, 2)))
S0, D = 0x1234567, 0x89AB
BATCHES = (1, 16)


def arg(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def limbs(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint64).reshape(-1, 4).copy()


def progression(q, g, first, step, n):
    """(first + i step) G for i < n as Montgomery limbs uint64[n, 8]: affine chord additions in Python integers"""
    def add(p, s):
        if p[0] == s[0]:
            lam = 3 * p[0] * p[0] * pow(2 * p[1], -1, q) % q
        else:
            lam = (s[1] - p[1]) * pow(s[0] - p[0], -1, q) % q
        x = (lam * lam - p[0] - s[0]) % q
        return (x, (lam * (p[0] - x) - p[1]) % q)

    def mul(k):
        acc = None
        for bit in bin(k)[2:]:
            acc = add(acc, acc) if acc else None
            if bit == "1":
                acc = add(acc, g) if acc else g
        return acc

    p, d, coords = mul(first), mul(step), []
    for _ in range(n):
        coords += [p[0] << 256, p[1] << 256]
        p = add(p, d)
    return limbs([v % q for v in coords]).reshape(n, 8)


def main():
    import torch
    dev = torch.device("cuda:0")
    eng = frw.WitnessEngine(0)
    launches = arg("--launches", 5)
    n = arg("--points", (1 << 18) - 1)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "msm_field.txt"), str)
    s0 = torch.cuda.current_stream().cuda_stream
    rng = random.Random(18)

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

    def uniform(r, batch):
        """-> (integers [batch][n], their Montgomery form on the device)"""
        row = [rng.randrange(r) for _ in range(n)]              # (a statement's scalars: the first one's times a unit, as uniform and quicker to make)
        ks = [row] + [[k * c % r for k in row] for c in (rng.randrange(2, r) for _ in range(batch - 1))]
        return ks, torch.from_numpy(limbs([k * (1 << 256) % r for row in ks for k in row]).view(np.int64).reshape(batch, n, 4)).to(dev)

    trace = arg("--trace", 0)
    if trace:
        name, q, r, b, g = CURVES[0]
        h = eng.msmf_load(q, r, b, progression(q, g, S0, D, n), frw.MSMF_POINTS_ARE_CHECKED)
        _, d_ks = uniform(r, trace)
        size = eng.msmf_workspace_bytes(h, trace)
        ws = torch.empty(size, dtype=torch.uint8, device=dev)
        out = torch.empty((trace, 8), dtype=torch.int64, device=dev)
        for _ in range(3):
            eng.msmf_dev(h, trace, d_ks, n, n, True, out, ws, size, s0)
        torch.cuda.synchronize()
        eng.msmf_free(h)
        eng.close()
        return

    times, shape = {}, {}
    for name, q, r, b, g in CURVES:
        h = eng.msmf_load(q, r, b, progression(q, g, S0, D, n))
        info = eng.msmf_info(h)
        shape[name] = (int(info.window_bits), int(info.num_windows), int(info.workspace_bytes_per_statement))
        gm = np.concatenate([limbs([g[0] * (1 << 256) % q]), limbs([g[1] * (1 << 256) % q])], axis=1)
        for batch in BATCHES:
            ks, d_ks = uniform(r, batch)
            size = eng.msmf_workspace_bytes(h, batch)
            ws = torch.empty(size, dtype=torch.uint8, device=dev)
            out = torch.empty((batch, 8), dtype=torch.int64, device=dev)
            times[name, batch] = timed(lambda: eng.msmf_dev(h, batch, d_ks, n, n, True, out, ws, size, s0))
            want = frw.curve_scalar_mul(q, r, b, np.repeat(gm, batch, axis=0), limbs([sum(k * (S0 + i * D) for i, k in enumerate(row)) % r for row in ks]))
            assert np.array_equal(out.cpu().numpy().view(np.uint64), want), "%s, batch %d: the sum is not the multiple of G it must be" % (name, batch)
            del ws, d_ks
        eng.msmf_free(h)

    yard = "BLS12-381 G1, dense bare handle"
    bases = eng.g1_fixed_base(limbs([rng.randrange(1, BLS12_381_FR) for _ in range(n)]))
    h = eng.msm_g1_load(bases, bare=True)
    per = int(eng.msm_info(h).workspace_bytes_per_signature)
    for batch in BATCHES:
        _, d_ks = uniform(BLS12_381_FR, batch)
        ws = torch.empty(batch * per, dtype=torch.uint8, device=dev)
        out = torch.empty((batch, 12), dtype=torch.int64, device=dev)
        times[yard, batch] = timed(lambda: eng.msm_g1_dev(h, batch, d_ks, n, True, out, ws, batch * per, s0))
        del ws, d_ks
    eng.msm_free(h)
    eng.close()

    lines = ["# tools/time_msm_field.py: n = %d points, uniform scalars below r in Montgomery form; HIP events, mean of %d back-to-back calls after a"
             % (n, launches),
             "# warm-up, one process; every frw_msmf_dev result equals the multiple of G it must be"]
    for name, _, _, _, _ in CURVES:
        lines.append("# %s: %d windows of %d bits, %.1f MB of workspace a statement" % (name, shape[name][1], shape[name][0], shape[name][2] / 1e6))
    for name in [c[0] for c in CURVES] + [yard]:
        call = "frw_msm_g1_dev" if name == yard else "frw_msmf_dev"
        for batch in BATCHES:
            t = times[name, batch]
            lines.append("%-14s %-32s batch %2d  %9.3f ms   %8.3f ms/statement   %7.2f ns/point" % (call + ",", name, batch, t * 1e3, t / batch * 1e3, t / batch / n * 1e9))
    for name, _, _, _, _ in CURVES:
        for batch in BATCHES:
            lines.append("ratio %-10s / yardstick, batch %2d   %6.2f" % (name, batch, times[name, batch] / times[yard, batch]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
