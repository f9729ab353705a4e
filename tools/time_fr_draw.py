"""Time the factor draw (frw_fr_draw_dev: fr_draw_kernel and the counter's step, falcon-r1cs_amd/csrc/frw_drbg.hip) on one MI355X, beside the
prover it feeds.  A record, judged against nothing: 8,192 scalars (the factors of a 4,096-proof call) and 2^20 scalars, and in the same
run one un-seeded frw_groth16_prove_rs_dev of 64 proofs of the cubic system of examples/custom_r1cs.py (I = 2, W = 3, C = 3, the 2^3
domain) -- HIP events around the call on the current stream, every buffer allocated beforehand, two warm-up calls, the median and the
minimum of five.  The first scalars of each draw are compared with hashlib before anything is timed.  One JSON object per line, also
written to --out (default profiles/r19_fr_draw.txt).
usage: python tools/time_fr_draw.py [reps=5] [--out PATH]"""
import hashlib
import json
import os
import random
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import falcon_r1cs_amd as frw
from custom_r1cs import R, montgomery, write_r1cs


def reference(seed, counter, tag, j):
    msg = b"FRW-FR-DRAW-001" + bytes([tag]) + seed + counter.to_bytes(8, "little") + j.to_bytes(8, "little")
    return int.from_bytes(hashlib.shake_256(msg).digest(64), "little") % R


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
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r19_fr_draw.txt")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    seed = bytes(range(32))
    d_seed = torch.from_numpy(np.frombuffer(seed, dtype=np.uint8).copy()).to(dev)
    lines = []
    for count in (8192, 1 << 20):
        d_counter = torch.zeros(1, dtype=torch.int64, device=dev)
        d_out = torch.empty((count, 4), dtype=torch.int64, device=dev)
        frw.fr_draw_dev(d_seed, d_counter, frw.DRAW_BLINDING, count, out=d_out, stream=stream)
        torch.cuda.synchronize()
        for j in (0, 1, count - 1):
            assert int.from_bytes(d_out[j].cpu().numpy().tobytes(), "little") == reference(seed, 0, 1, j), j
        med, lo = event_ms(lambda: frw.fr_draw_dev(d_seed, d_counter, frw.DRAW_BLINDING, count, out=d_out, stream=stream), reps)
        lines.append(json.dumps({"what": "frw_fr_draw_dev (the draw and the counter's step)", "scalars": count, "reps": reps,
                                 "ms_median": round(med, 4), "ms_min": round(lo, 4), "scalars_per_second": round(count / (med * 1e-3))}))
        print(lines[-1], flush=True)
    # the prover it feeds: 64 proofs of the cubic system in one un-seeded call
    eng = frw.WitnessEngine(0)
    ONE, Y, X, X2, X3 = range(5)
    a = [[(1, X)], [(1, X2)], [(1, X3), (1, X), (5, ONE)]]
    b = [[(1, X)], [(1, X)], [(1, ONE)]]
    c = [[(1, X2)], [(1, X3)], [(1, Y)]]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cubic.r1cs")
        write_r1cs(path, 2, 3, (a, b, c))
        r1cs = eng.r1cs_load_file(path)
    rng = random.Random(19)
    key, _ = eng.groth16_setup_r1cs(r1cs, *(rng.randrange(2, R) for _ in range(5)))
    batch = 64
    xs = [rng.randrange(R) for _ in range(batch)]
    wit = torch.cat([montgomery([x, x * x, x ** 3]) for x in xs]).to(dev)
    inst = torch.cat([montgomery([1, x ** 3 + x + 5]) for x in xs]).to(dev)
    d_counter = torch.zeros(1, dtype=torch.int64, device=dev)
    d_rs = frw.fr_draw_dev(d_seed, d_counter, frw.DRAW_BLINDING, 2 * batch, stream=stream).reshape(batch, 2, 4)
    ws_bytes = eng.groth16_workspace_bytes(key, r1cs, batch)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    proofs = torch.empty((batch, 48), dtype=torch.int64, device=dev)
    bad = torch.empty(batch, dtype=torch.int32, device=dev)
    med, lo = event_ms(lambda: eng.groth16_prove_rs_dev(key, r1cs, batch, wit, inst, d_rs, proofs, ws, ws_bytes, bad, stream), reps)
    assert not bad.any(), "the witness violates the system"
    dmed, dlo = event_ms(lambda: frw.fr_draw_dev(d_seed, d_counter, frw.DRAW_BLINDING, 2 * batch, out=d_rs, stream=stream), reps)
    lines.append(json.dumps({"what": "frw_groth16_prove_rs_dev, cubic system, un-seeded, beside the draw of its 128 factors", "proofs_per_call": batch,
                             "reps": reps, "prove_ms_median": round(med, 3), "prove_ms_min": round(lo, 3), "draw_ms_median": round(dmed, 4),
                             "draw_ms_min": round(dlo, 4), "draw_share_of_prove": round(dmed / med, 4)}))
    print(lines[-1], flush=True)
    eng.groth16_pk_free(key)
    eng.r1cs_free(r1cs)
    eng.close()
    with open(out, "w") as f:
        f.write("# python tools/time_fr_draw.py %d   (one MI355X; HIP events, medians and minima of %d; a record, judged against nothing)\n" % (reps, reps))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
