"""Time Groth16 verification on the host (frw_groth16_verify) against the device path (frw_groth16_vk_load_dev,
frw_groth16_prepare_inputs_dev, frw_groth16_verify_dev).  One JSON object per case:
  (a) 64 Falcon-1024 per-signature proofs (frw_groth16_setup + frw_groth16_prove_dev)
  (b) 64 proofs against one 32,769-input key (a sixteen-statement aggregate's size)
  (c) one proof with 1,571,841 inputs (the 1,024-statement aggregate's)
  (f) the whole verification on the device (frw_groth16_verify_full_dev) of Falcon-1024 per-signature proofs at 1, 64, 1,024, 4,096 and
      16,384 proofs (64 proofs made, tiled), per proof and batched (FRW_VERIFY_BATCHED: one final exponentiation per pass), proofs/s
      next to the host (frw_groth16_verify) and verify_dev columns -- those two up to
      1,024 proofs: beyond that the host's pairings alone take many seconds a repetition
(b) and (c) are statements made in the exponent (tests/test_gpu_verify_dev.py: gamma_abc_g1[i] = g_i G1 from the oracle's fixed-base
multiples, A = a G1, B = b G2, C solved for), 14-bit inputs.  Key loads: host with every point checked, host vouched
(FRW_VK_POINTS_ARE_CHECKED), device (every point checked there).
  --wire  4,096 Falcon-1024 proofs through frw_groth16_verify_wire_dev (compressed and uncompressed wire bytes) against
      frw_groth16_verify_full_dev on limbs in the same process, HIP-event medians; the encode and the decode alone; the
      1,571,841-input key loaded by frw_groth16_vk_load_wire_dev against frw_groth16_vk_load_dev
usage: python tools/time_verify.py [a|b|c|f ...] [--wire] [reps=3]"""
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import falcon_r1cs_amd as frw
import frw_testlib as T
import test_gpu_verify_dev as V

R = V.R


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t


def falcon_case(batch=64, logn=10):
    dev = torch.device("cuda:0")
    eng = frw.WitnessEngine(0)
    L = frw.layout(logn)
    rng = random.Random(5)
    pk, vk = eng.groth16_setup(0, logn, *(rng.randrange(2, R) for _ in range(5)))
    r1cs = eng.r1cs_load(0, logn)
    sig, pk_, hm = frw.synth_triples(logn, batch, seed=1)
    d = [torch.from_numpy(a.view(np.int16)).to(dev) for a in (sig, pk_, hm)]
    wit = torch.empty((batch, L.num_witness, 4), dtype=torch.int64, device=dev)
    inst = torch.empty((batch, L.num_instance, 4), dtype=torch.int64, device=dev)
    st = torch.empty(batch, dtype=torch.int32, device=dev)
    eng.witness_ntt_verify_dev(logn, batch, d[0], d[1], d[2], wit, inst, st, frw.ENC_MONTGOMERY, 0)
    rs = np.array([T.ints_to_limbs([rng.randrange(R), rng.randrange(R)]) for _ in range(batch)])
    ws_bytes = eng.groth16_workspace_bytes(pk, r1cs, batch)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    proofs = torch.empty((batch, 48), dtype=torch.int64, device=dev)
    eng.groth16_prove_dev(pk, r1cs, batch, wit, inst, rs, proofs, ws, ws_bytes, None, 0)
    torch.cuda.synchronize()
    del wit, ws
    eng.r1cs_free(r1cs)
    eng.groth16_pk_free(pk)
    flat = np.concatenate([np.asarray(vk[k], dtype=np.uint64).reshape(-1) for k in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1")])
    return "a: %d Falcon-%d proofs" % (batch, 1 << logn), flat, inst, proofs


def exponent_case(oracle, n, batch):
    k = V.Key(oracle, n, seed=n)
    rng = random.Random(n)
    rs = np.random.default_rng(n)
    insts, proofs = [], []
    for _ in range(batch):
        small = rs.integers(0, 1 << 14, n)
        small[0] = 1
        proofs.append(V.proof_limbs(k.proof(k.dot(small, {}), rng)))
        insts.append(V.encode(small, {}, True))
    name = "%s: %d proof%s against a %d-input key" % ("b" if batch > 1 else "c", batch, "s" if batch > 1 else "", n)
    return name, k.limbs(), V._dev(np.stack(insts)), V._dev(np.stack(proofs))


def run(name, vk, d_inst, d_proofs, reps):
    batch = d_proofs.shape[0]
    inst_h, proofs_h = d_inst.cpu().numpy().view(np.uint64), d_proofs.cpu().numpy().view(np.uint64)
    host, load_full = timed(lambda: frw.Groth16Verifier(vk))
    vouched, load_vouched = timed(lambda: frw.Groth16Verifier(vk, points_are_checked=True))
    vouched.close()
    devk, load_dev = timed(lambda: frw.Groth16Verifier(vk, device=0))
    ws = torch.empty(devk.workspace_bytes(batch), dtype=torch.uint8, device=d_inst.device)
    devk.prepare_inputs_dev(d_inst, workspace=ws)                         # (warm-up)
    torch.cuda.synchronize()
    prep = []
    for _ in range(reps):
        t = time.perf_counter()
        devk.prepare_inputs_dev(d_inst, workspace=ws)
        torch.cuda.synchronize()
        prep.append(time.perf_counter() - t)
    host_s, dev_s = [], []
    for _ in range(reps):
        h, s = timed(lambda: host.verify(inst_h, proofs_h))
        host_s.append(s)
        d, s = timed(lambda: devk.verify_dev(d_inst, d_proofs, workspace=ws))
        dev_s.append(s)
        assert h.tolist() == d.tolist(), (h, d)
    out = {"case": name, "num_instance": host.num_instance, "batch": batch, "accepted": int((d == 1).sum()),
           "vk_load_s": {"host_checked": round(load_full, 4), "host_vouched": round(load_vouched, 4), "device_checked": round(load_dev, 4)},
           "prepare_inputs_dev_ms": {"min": round(1e3 * min(prep), 3), "median": round(1e3 * sorted(prep)[len(prep) // 2], 3)},
           "verify_s": {"host_min": round(min(host_s), 4), "device_min": round(min(dev_s), 4),
                        "host_median": round(sorted(host_s)[len(host_s) // 2], 4), "device_median": round(sorted(dev_s)[len(dev_s) // 2], 4)},
           "workspace_bytes": int(ws.numel())}
    host.close()
    devk.close()
    print(json.dumps(out), flush=True)


def full_leg(reps, sizes=(1, 64, 1024, 4096, 16384), host_up_to=1024):
    name, vk, inst, proofs = falcon_case()
    devk = frw.Groth16Verifier(vk, device=0)
    host = frw.Groth16Verifier(vk)
    for n in sizes:
        idx = torch.arange(n, device=inst.device) % inst.shape[0]
        d_inst, d_proofs = inst[idx].contiguous(), proofs[idx].contiguous()
        ws = torch.empty(devk.full_workspace_bytes(n), dtype=torch.uint8, device=inst.device)
        got = devk.verify_full_dev(d_inst, d_proofs, workspace=ws)          # (warm-up)
        torch.cuda.synchronize()
        assert int((got == 1).sum()) == n
        full = []
        for _ in range(reps):
            t = time.perf_counter()
            devk.verify_full_dev(d_inst, d_proofs, workspace=ws)
            torch.cuda.synchronize()
            full.append(time.perf_counter() - t)
        wsb = torch.empty(devk.full_workspace_bytes(n, frw.VERIFY_BATCHED), dtype=torch.uint8, device=inst.device)
        passed = torch.zeros(1, dtype=torch.int32, device=inst.device)
        got_b = devk.verify_full_dev(d_inst, d_proofs, batched=True, workspace=wsb, batch_passed=passed)   # (warm-up)
        torch.cuda.synchronize()
        assert got_b.cpu().tolist() == got.cpu().tolist() and passed.item() == 1
        batched = []
        for _ in range(reps):
            t = time.perf_counter()
            devk.verify_full_dev(d_inst, d_proofs, batched=True, workspace=wsb, batch_passed=passed)
            torch.cuda.synchronize()
            batched.append(time.perf_counter() - t)
        out = {"case": "f: %d Falcon-1024 proofs, verify_full_dev" % n, "batch": n, "num_instance": devk.num_instance,
               "full_dev_ms": {"min": round(1e3 * min(full), 3), "median": round(1e3 * sorted(full)[len(full) // 2], 3)},
               "full_dev_proofs_per_s": round(n / min(full), 1),
               "batched_ms": {"min": round(1e3 * min(batched), 3), "median": round(1e3 * sorted(batched)[len(batched) // 2], 3)},
               "batched_proofs_per_s": round(n / min(batched), 1), "workspace_bytes": int(ws.numel())}
        del ws, wsb
        if n <= host_up_to:
            inst_h, proofs_h = d_inst.cpu().numpy().view(np.uint64), d_proofs.cpu().numpy().view(np.uint64)
            wsd = torch.empty(devk.workspace_bytes(n), dtype=torch.uint8, device=inst.device)
            h, hs = timed(lambda: host.verify(inst_h, proofs_h))
            d, ds = timed(lambda: devk.verify_dev(d_inst, d_proofs, workspace=wsd))
            assert h.tolist() == d.tolist() == got.cpu().tolist()
            out["host_proofs_per_s"] = round(n / hs, 1)
            out["verify_dev_proofs_per_s"] = round(n / ds, 1)
            del wsd
        print(json.dumps(out), flush=True)
        torch.cuda.empty_cache()
    devk.close()
    host.close()


def event_ms(fn, reps):
    """HIP-event times of fn() on the current stream, in ms: (median, min), after two warm-ups.  fn is the C entry point alone: its
    outputs are allocated before the timing, not inside it."""
    fn()
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return round(sorted(times)[len(times) // 2], 3), round(min(times), 3)


def wire_leg(oracle, reps, n=4096):
    """--wire: verification from ark-serialize's bytes (frw_groth16_verify_wire_dev) against the limbs path (frw_groth16_verify_full_dev)
    in the same process, the decode alone, and a key loaded from bytes against the same key loaded from limbs.  The timed calls are the
    C entry points with every output allocated beforehand; the codec alone (well under a millisecond) gets five times the repetitions."""
    import ctypes as C
    reps = max(reps, 11)
    short_reps = 5 * reps
    name, vk, inst, proofs = falcon_case()
    devk = frw.Groth16Verifier(vk, device=0)
    lib, dev = frw.load_library(), inst.device
    idx = torch.arange(n, device=dev) % inst.shape[0]
    d_inst, d_proofs = inst[idx].contiguous(), proofs[idx].contiguous()
    s0 = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(devk.wire_workspace_bytes(n, 0, False), dtype=torch.uint8, device=dev)
    verdicts = torch.empty(n, dtype=torch.int32, device=dev)
    back = torch.empty((n, 48), dtype=torch.int64, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def call(rc):
        if rc:
            raise RuntimeError("frw call failed: %d" % rc)

    def verify_limbs():
        call(lib.frw_groth16_verify_full_dev(devk._h, n, ptr(d_inst), frw.ENC_MONTGOMERY, ptr(d_proofs), 0, None, ptr(verdicts), None, ptr(ws),
                                             ws.numel(), C.c_void_p(s0)))

    limbs = event_ms(verify_limbs, reps)
    assert int((verdicts == 1).sum()) == n
    out = {"case": "wire: %d Falcon-1024 proofs" % n, "batch": n, "reps": reps, "codec_reps": short_reps,
           "timed": "C entry points, outputs allocated beforehand, HIP events on one stream",
           "verify_full_dev_limbs_ms": {"median": limbs[0], "min": limbs[1]}}
    for compressed in (True, False):
        tag, mode = ("compressed", 0) if compressed else ("uncompressed", 1)
        d_wire = torch.empty((n, frw.proof_wire_bytes(compressed)), dtype=torch.uint8, device=dev)
        enc = event_ms(lambda: call(lib.frw_groth16_proofs_to_wire_dev(0, n, ptr(d_proofs), mode, ptr(d_wire), ptr(st), C.c_void_p(s0))), short_reps)
        assert not st.any().item()
        dec = event_ms(lambda: call(lib.frw_groth16_proofs_from_wire_dev(0, n, ptr(d_wire), mode, ptr(back), ptr(st), C.c_void_p(s0))), short_reps)
        assert bool((back == d_proofs).all()) and not st.any().item()
        verdicts.zero_()
        ver = event_ms(lambda: call(lib.frw_groth16_verify_wire_dev(devk._h, n, ptr(d_inst), frw.ENC_MONTGOMERY, ptr(d_wire), mode, 0, None,
                                                                    ptr(verdicts), None, ptr(ws), ws.numel(), C.c_void_p(s0))), reps)
        assert int((verdicts == 1).sum()) == n
        out[tag] = {"encode_ms": {"median": enc[0], "min": enc[1]}, "decode_ms": {"median": dec[0], "min": dec[1]},
                    "verify_wire_dev_ms": {"median": ver[0], "min": ver[1]}, "over_limbs": round(ver[0] / limbs[0], 3),
                    "proofs_per_s": round(n / (1e-3 * ver[0]), 1)}
    # (the limbs path once more, after the wire runs: drift shows here)
    again = event_ms(verify_limbs, reps)
    out["verify_full_dev_limbs_again_ms"] = {"median": again[0], "min": again[1]}
    devk.close()
    print(json.dumps(out), flush=True)
    del ws, d_inst, d_proofs
    torch.cuda.empty_cache()
    # the largest key this tool uses: loaded from limbs and from bytes, every point checked on the device both ways
    k = V.key(oracle, V.BIG)
    flat = k.limbs()
    out = {"case": "wire: a key of %d inputs" % V.BIG, "num_instance": V.BIG}
    h, s = timed(lambda: frw.Groth16Verifier(flat, device=0))
    h.close()
    loads = []
    for _ in range(3):
        h, s = timed(lambda: frw.Groth16Verifier(flat, device=0))
        h.close()
        loads.append(s)
    out["vk_load_dev_s"] = {"median": round(sorted(loads)[1], 4), "min": round(min(loads), 4)}
    for compressed in (True, False):
        data, s = timed(lambda: frw.vk_to_wire(flat, compressed))
        loads = []
        for _ in range(3):
            h, t = timed(lambda: frw.Groth16Verifier.from_wire(data, device=0, compressed=compressed))
            h.close()
            loads.append(t)
        out["compressed" if compressed else "uncompressed"] = {"bytes": len(data), "vk_to_wire_host_s": round(s, 4),
                                                               "vk_load_wire_dev_s": {"median": round(sorted(loads)[1], 4), "min": round(min(loads), 4)}}
    print(json.dumps(out), flush=True)


def main():
    if "--wire" in sys.argv:
        sys.argv = [a for a in sys.argv if a != "--wire"] + ["wire"]
    args = [a for a in sys.argv[1:] if not a.isdigit()] or ["a", "b", "c"]
    reps = int(next((a for a in sys.argv[1:] if a.isdigit()), 3))
    oracle = T.load_oracle()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "host_threads": os.cpu_count(), "reps": reps}), flush=True)
    for c in args:
        if c == "a":
            run(*falcon_case(), reps)
        elif c == "b":
            run(*exponent_case(oracle, 32769, 64), reps)
        elif c == "c":
            run(*exponent_case(oracle, V.BIG, 1), reps)
        elif c == "f":
            full_leg(reps)
        elif c == "wire":
            wire_leg(oracle, reps)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
