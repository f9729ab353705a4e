"""Time the re-randomisation of Groth16 proofs on one MI355X (frw_groth16_rerandomize_dev / _wire_dev): 1, 64, 4,096 and
16,384 proofs per call with the subgroup checks and with the points vouched for (the difference is the checks' share), the wire form
(compressed) at 4,096, and the host function on one core.  The proofs are random points A = a G1, B = b G2, C = c G1 under a synthetic
key (the chains' time does not depend on the statement; a key's size does not enter), the factors uniform below 2^256.
The timed calls are the C entry points with every buffer allocated beforehand; HIP events on one stream around one call.  Before
anything is timed the device's output for 64 proofs is compared with the host function's, bit for bit.  The kernels' shares come from a
separate run under `rocprofv3 --kernel-trace --stats -- python tools/time_rerandomize.py 3 --sizes 4096` (their names start with
rerand_).  One JSON object per line, also written to --out (default profiles/r14_rerandomize.txt).
usage: python tools/time_rerandomize.py [reps=7] [--sizes 1,64,4096,16384] [--out PATH]"""
import ctypes as C
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import falcon_r1cs_amd as frw

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def ptr(t):
    return C.c_void_p(t.data_ptr())


def call(rc):
    if rc:
        raise RuntimeError("frw call failed: %d (%s)" % (rc, frw.load_library().frw_last_error().decode()))


def event_ms(fn, reps):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return {"median": round(sorted(times)[len(times) // 2], 3), "min": round(min(times), 3)}


def scalars(rng, count, below=R):
    return np.frombuffer(b"".join(rng.randrange(1, below).to_bytes(32, "little") for _ in range(count)), dtype=np.uint64).reshape(count, 4).copy()


def main():
    argv = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "r14_rerandomize.txt")
    sizes = [1, 64, 4096, 16384]
    for flag in ("--out", "--sizes"):
        if flag in argv:
            i = argv.index(flag)
            if flag == "--out":
                out = argv[i + 1]
            else:
                sizes = [int(s) for s in argv[i + 1].split(",")]
            del argv[i:i + 2]
    reps = int(argv[0]) if argv else 7
    dev = torch.device("cuda:0")
    eng = frw.WitnessEngine(0)
    lib = frw.load_library()
    rng = random.Random(14)
    top = max(sizes + [64])
    # the key: alpha G1 | beta, gamma, delta G2 | three gamma_abc_g1 points; the proofs: a G1 | b G2 | c G1
    g1 = eng.g1_fixed_base(scalars(rng, 4 + 2 * top))
    g2 = eng.g2_fixed_base(scalars(rng, 3 + top))
    vk = np.concatenate([g1[0], g2[0], g2[1], g2[2], g1[1:4].reshape(-1)])
    ver = frw.Groth16Verifier(vk, device=0)
    proofs = np.concatenate([g1[4:4 + top], g2[3:], g1[4 + top:]], axis=1)
    factors = scalars(rng, 2 * top, 1 << 256).reshape(top, 2, 4)
    d_proofs = torch.from_numpy(proofs.view(np.int64)).to(dev)
    d_factors = torch.from_numpy(factors.view(np.int64)).to(dev)
    s0 = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_out = torch.empty((top, 48), dtype=torch.int64, device=dev)
    d_status = torch.empty(top, dtype=torch.int32, device=dev)
    ws = torch.empty(ver.rerandomize_workspace_bytes(top, frw.engine.WIRE_COMPRESSED), dtype=torch.uint8, device=dev)

    def limbs(n, flags):
        call(lib.frw_groth16_rerandomize_dev(ver._h, n, ptr(d_proofs), ptr(d_factors), flags, ptr(d_out), ptr(d_status), ptr(ws), ws.numel(), s0))

    # what is timed is what was checked: 64 proofs against the host function
    want, want_status = ver.rerandomize(proofs[:64], factors[:64])
    for flags in (0, frw.VERIFY_POINTS_ARE_CHECKED):
        limbs(64, flags)
        torch.cuda.synchronize()
        assert d_status[:64].tolist() == want_status.tolist() == [0] * 64
        assert np.array_equal(d_out[:64].cpu().numpy().view(np.uint64), want), "the device's proofs differ from the host's"
    lines = [json.dumps({"tool": "tools/time_rerandomize.py", "device": torch.cuda.get_device_name(0), "reps": reps,
                         "timed": "C entry points, buffers allocated beforehand, HIP events on one stream around one call; ms per call",
                         "checked": "64 proofs equal frw_groth16_rerandomize's, bit for bit, with and without the vouching flag"})]
    for n in sizes:
        limbs(n, 0)
        limbs(n, 1)
        torch.cuda.synchronize()
        t = [event_ms(lambda: limbs(n, 0), reps), event_ms(lambda: limbs(n, 1), reps), event_ms(lambda: limbs(n, 0), reps),
             event_ms(lambda: limbs(n, 1), reps)]
        full, vouched = min(t[0]["median"], t[2]["median"]), min(t[1]["median"], t[3]["median"])
        lines.append(json.dumps({"case": "%d proofs, rerandomize_dev" % n, "batch": n, "checked_ms": t[0], "vouched_ms": t[1], "checked_again_ms": t[2],
                                 "vouched_again_ms": t[3], "proofs_per_s": round(n / full * 1e3, 1), "vouched_proofs_per_s": round(n / vouched * 1e3, 1),
                                 "subgroup_checks_share": round(1 - vouched / full, 3)}))
        print(lines[-1], flush=True)
    if 4096 in sizes:
        n = 4096
        wire_in, st = frw.proofs_to_wire_dev(d_proofs[:n], True, s0.value)
        d_wire_out = torch.empty_like(wire_in)
        torch.cuda.synchronize()
        assert not st.any().item()

        def wire():
            call(lib.frw_groth16_rerandomize_wire_dev(ver._h, n, ptr(wire_in), 0, ptr(d_factors), 0, ptr(d_wire_out), ptr(d_status), ptr(ws), ws.numel(), s0))

        wire()
        limbs(n, 0)
        torch.cuda.synchronize()
        again, st = frw.proofs_to_wire_dev(d_out[:n], True, s0.value)
        torch.cuda.synchronize()
        assert torch.equal(again, d_wire_out), "the wire form's bytes differ from the encoded limb form's"
        lines.append(json.dumps({"case": "%d proofs, rerandomize_wire_dev, compressed in and out" % n, "batch": n, "wire_ms": event_ms(wire, reps),
                                 "limbs_ms": event_ms(lambda: limbs(n, 0), reps), "bytes_equal": True}))
        print(lines[-1], flush=True)
    # the host function: one proof, hence one thread
    host = []
    for i in range(5):
        t0 = time.perf_counter()
        ver.rerandomize(proofs[i:i + 1], factors[i:i + 1])
        host.append((time.perf_counter() - t0) * 1e3)
    host_v = []
    for i in range(5):
        t0 = time.perf_counter()
        ver.rerandomize(proofs[i:i + 1], factors[i:i + 1], frw.VERIFY_POINTS_ARE_CHECKED)
        host_v.append((time.perf_counter() - t0) * 1e3)
    lines.append(json.dumps({"case": "frw_groth16_rerandomize, one proof on one core", "ms": round(sorted(host)[2], 3),
                             "vouched_ms": round(sorted(host_v)[2], 3)}))
    print(lines[-1], flush=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    ver.close()
    eng.close()


if __name__ == "__main__":
    main()
