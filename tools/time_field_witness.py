"""Time the witness kernel over a field registered at run time against its hard-wired FRW_ENC_MONTGOMERY instantiation: the benchmark's
launch shape (Falcon-1024, 32,768 signatures per launch), ONE output buffer reused by every launch, the two encodings alternating launch
by launch in one process, each launch between its own pair of HIP events.  The margin the new encoding is held to is
FRW_ENC_MONTGOMERY's own spread across its repetitions in the same run.  One JSON object per line; the last one is the verdict.

usage: python tools/time_field_witness.py [--signatures 32768] [--logn 10] [--launches 12] [--warmup 2] [--modulus HEX]"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import falcon_r1cs_amd as frw

BN254_FR = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
say = lambda **kw: print(json.dumps(kw), flush=True)


def arg(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    import torch
    dev = torch.device("cuda:0")
    logn, batch = arg("--logn", 10), arg("--signatures", 32768)
    launches, warmup = max(arg("--launches", 12), 10), arg("--warmup", 2)
    p = arg("--modulus", BN254_FR, lambda s: int(s, 16))
    eng = frw.WitnessEngine(0)
    L = frw.layout(logn)
    field = eng.field_encoding(p)
    encodings = (("montgomery", frw.ENC_MONTGOMERY), ("field", field))
    sig, pk, hm = frw.synth_triples(logn, batch, seed=2026)
    d = [torch.from_numpy(a.view(np.int16)).to(dev) for a in (sig, pk, hm)]
    wit = torch.empty((batch, L.num_witness, 4), dtype=torch.int64, device=dev)
    inst = torch.empty((batch, L.num_instance, 4), dtype=torch.int64, device=dev)
    st = torch.empty(batch, dtype=torch.int32, device=dev)
    s0 = torch.cuda.current_stream().cuda_stream
    nbytes = batch * (L.num_witness + L.num_instance) * 32
    say(logn=logn, signatures=batch, bytes_per_launch=nbytes, modulus=hex(p), launch_shape={k: eng.launch_shape(logn, batch, e) for k, e in encodings})

    def launch(enc):
        eng.witness_ntt_verify_dev(logn, batch, d[0], d[1], d[2], wit, inst, st, enc, s0)

    for _ in range(warmup):
        for _, enc in encodings:
            launch(enc)
    torch.cuda.synchronize()
    events = {k: [] for k, _ in encodings}
    for _ in range(launches):
        for k, enc in encodings:                                 # alternating: both see the same clocks and the same neighbours
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch(enc)
            b.record()
            events[k].append((a, b))
    torch.cuda.synchronize()
    assert not st.any()
    ms = {k: [a.elapsed_time(b) for a, b in v] for k, v in events.items()}
    out = {}
    for k, v in ms.items():
        med = statistics.median(v)
        out[k] = {"median_ms": med, "min_ms": min(v), "max_ms": max(v), "spread": (max(v) - min(v)) / med,
                  "signatures_per_s": batch / med * 1e3, "GB_per_s": nbytes / med / 1e6}
        say(encoding=k, launches=len(v), ms=[round(x, 3) for x in v], **out[k])
    slower = out["field"]["median_ms"] / out["montgomery"]["median_ms"] - 1.0
    say(field_slower_by=slower, margin_montgomery_spread=out["montgomery"]["spread"], within_margin=slower <= out["montgomery"]["spread"])
    eng.close()


if __name__ == "__main__":
    main()
