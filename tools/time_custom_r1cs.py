"""Time Groth16 proofs of a constraint system that came in as matrices, on a domain below 2^14 (frw_r1cs_load_csr, frw_qap_small.hip), on
one MI355X.  A record, judged against nothing: a seeded satisfied system of 4,091 rows and 5 instance variables (C + I = 4,096, the 2^12
domain: the largest whose arrays stay in LDS), a key from frw_groth16_setup_r1cs, and frw_groth16_prove_dev for 1 proof and for 64 in one
call -- HIP events around the call on the current stream, every buffer allocated beforehand, two warm-up calls, the median and the
minimum of five.  The witness map alone (frw_qap_witness_map_dev) is timed the same way.  One JSON object per line, also written to --out
(default profiles/r18_custom_r1cs.txt).
usage: python tools/time_custom_r1cs.py [reps=5] [--out PATH]"""
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import falcon_r1cs_amd as frw

P = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
NI, NC, FREE = 5, 4091, 4


def limbs(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint64).reshape(-1, 4).copy()


def value(rng):
    return rng.randrange(1, 1 << 14) if rng.random() < 0.5 else rng.randrange(1 << 250, P)


def rows(rng):
    """row i: sparse A_i, B_i over the variables that exist, C_i = a coefficient times a fresh witness variable"""
    coeffs = [1, P - 1, 2] + [value(rng) for _ in range(9)]
    a, b, c = [], [], []
    for row in range(NC):
        existing = NI + FREE + row
        a.append([(rng.choice(coeffs), rng.randrange(existing)) for _ in range(rng.randrange(1, 4))])
        b.append([(rng.choice(coeffs), rng.randrange(existing)) for _ in range(rng.randrange(1, 3))])
        c.append([(rng.choice(coeffs), existing)])
    return a, b, c


def assignment(mats, rng):
    z = [1] + [value(rng) for _ in range(NI - 1 + FREE)]
    dot = lambda row: sum(k * z[col] for k, col in row) % P
    for ra, rb, rc in zip(*mats):
        z.append(dot(ra) * dot(rb) * pow(rc[0][0], -1, P) % P)
    return z


def event_ms(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(min(times))


def main():
    args = [x for x in sys.argv[1:] if not x.startswith("--")]
    reps = int(args[0]) if args else 5
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r18_custom_r1cs.txt")
    rng = random.Random(16)
    mats = rows(rng)
    csr = [(np.cumsum([0] + [len(r) for r in m]).astype(np.uint64), np.array([col for r in m for _, col in r], dtype=np.uint32),
            limbs([k for r in m for k, _ in r])) for m in mats]
    eng = frw.WitnessEngine(0)
    dev = torch.device("cuda:0")
    handle = eng.r1cs_load_csr(NI, FREE + NC, csr)
    key, _ = eng.groth16_setup_r1cs(handle, *(rng.randrange(2, P) for _ in range(5)))
    lines = []
    stream = torch.cuda.current_stream().cuda_stream
    q = eng.qap_info(handle)
    for batch in (1, 64):
        zs = [assignment(mats, rng) for _ in range(batch)]
        mont = lambda vals: limbs([v * (1 << 256) % P for v in vals])
        wit = torch.from_numpy(np.stack([mont(z[NI:]) for z in zs]).view(np.int64)).to(dev)
        inst = torch.from_numpy(np.stack([mont(z[:NI]) for z in zs]).view(np.int64)).to(dev)
        rs = np.stack([limbs([rng.randrange(P), rng.randrange(P)]) for _ in range(batch)])
        ws_bytes = eng.groth16_workspace_bytes(key, handle, batch)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        proofs = torch.empty((batch, 48), dtype=torch.int64, device=dev)
        bad = torch.empty(batch, dtype=torch.int32, device=dev)
        prove = lambda: eng.groth16_prove_dev(key, handle, batch, wit, inst, rs, proofs, ws, ws_bytes, bad, stream)
        med, lo = event_ms(prove, reps)
        assert not bad.any(), "the generated witness violates the system"
        qws = torch.empty(batch * int(q.workspace_bytes_per_signature), dtype=torch.uint8, device=dev)
        h = torch.empty((batch, int(q.domain_size), 4), dtype=torch.int64, device=dev)
        wmap = lambda: eng.qap_witness_map_dev(handle, batch, wit, inst, h, qws, qws.numel(), bad, stream)
        wmed, wlo = event_ms(wmap, reps)
        lines.append(json.dumps({"what": "frw_groth16_prove_dev, custom system", "constraints": NC, "instance": NI, "witness": FREE + NC,
                                 "log_domain": int(q.log_domain_size), "proofs_per_call": batch, "reps": reps, "prove_ms_median": round(med, 3),
                                 "prove_ms_min": round(lo, 3), "witness_map_ms_median": round(wmed, 3), "witness_map_ms_min": round(wlo, 3)}))
        print(lines[-1], flush=True)
    eng.groth16_pk_free(key)
    eng.r1cs_free(handle)
    eng.close()
    with open(out, "w") as f:
        f.write("# python tools/time_custom_r1cs.py %d   (one MI355X; HIP events, medians and minima of %d; a record, judged against nothing)\n" % (reps, reps))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
