"""Time the schoolbook witness kernel against the device's compute-free write stream, in one process and on one buffer:
HIP-event time of back-to-back frw_witness_schoolbook_verify_dev launches (Falcon-1024, and Falcon-512 at the same byte
count) and of frw_diag_write_stream_dev over the same bytes.  The batch is sized so that one launch lasts at least 25 ms at
the write stream's rate (4,096 Falcon-1024 signatures = 151 GB; DESIGN 5.1: launch duration decides the rate), or by the
device's free memory where that is less; --signatures overrides it.  One JSON object per line: GB/s, the fraction of the
stream, witnesses/s.
  --lib PATH    time the kernels of another build of the library (e.g. one compiled with -DFRW_NO_STORE: the instruction time
                alone, which says which side binds); inputs and layouts still come from the package's own library
  --prover      instead: wall time of the checked frw_r1cs_load of both handles, of frw_groth16_setup and of
                frw_groth16_prove_dev + frw_groth16_verify for Falcon-512 (--proof1024: the same once for Falcon-1024)
usage: python tools/time_schoolbook.py [--signatures K] [--launches 5] [--lib PATH] | --prover [--proof1024]"""
import ctypes as C
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import falcon_r1cs_amd as frw

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
say = lambda **kw: print(json.dumps(kw), flush=True)


def arg(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def other_build(path):
    """(library, context) of another build, with the two entry points timed here."""
    lib = C.CDLL(os.path.abspath(path))
    lib.frw_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.frw_witness_schoolbook_verify_dev.argtypes = [C.c_void_p, C.c_int, C.c_size_t] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 4
    lib.frw_diag_write_stream_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    ctx = C.c_void_p()
    assert lib.frw_ctx_create(0, C.byref(ctx)) == 0
    return lib, ctx


def kernel_rates():
    import torch
    dev = torch.device("cuda:0")
    eng = frw.WitnessEngine(0)
    launches = arg("--launches", 5)
    lib_path = arg("--lib", None, str)
    other = other_build(lib_path) if lib_path else None
    L10 = frw.layout_schoolbook(10)
    free_b, _ = torch.cuda.mem_get_info()
    k10 = arg("--signatures", min(4096, int(free_b * 0.9) // (L10.num_witness * 32 + L10.num_instance * 32 + 3 * 2048)))
    nbytes = k10 * L10.num_witness * 32
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)

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

    s0 = torch.cuda.current_stream().cuda_stream
    for logn in (10, 9):
        L = frw.layout_schoolbook(logn)
        k = nbytes // (L.num_witness * 32)
        used = k * L.num_witness * 32
        sig, pk, hm = frw.synth_triples(logn, min(k, 64), seed=5)
        rep = (k + sig.shape[0] - 1) // sig.shape[0]
        d = [torch.from_numpy(np.tile(a, (rep, 1))[:k].copy().view(np.int16)).to(dev) for a in (sig, pk, hm)]
        inst = torch.empty((k, L.num_instance, 4), dtype=torch.int64, device=dev)
        st = torch.empty(k, dtype=torch.int32, device=dev)
        if other:
            lib, ctx = other
            P = lambda t: C.c_void_p(t.data_ptr())
            stream = lambda: lib.frw_diag_write_stream_dev(ctx, P(buf), used, L.num_witness * 32, C.c_void_p(s0))
            kern = lambda: lib.frw_witness_schoolbook_verify_dev(ctx, logn, k, P(d[0]), P(d[1]), P(d[2]), frw.ENC_MONTGOMERY, P(buf), P(inst),
                                                                 P(st), C.c_void_p(s0))
            assert kern() == 0 and stream() == 0
        else:
            stream = lambda: eng.diag_write_stream_dev(buf, used, L.num_witness * 32, s0)
            kern = lambda: eng.witness_schoolbook_verify_dev(logn, k, d[0], d[1], d[2], buf, inst, st, frw.ENC_MONTGOMERY, s0)
        t_w = timed(stream)
        t_k = timed(kern)
        assert int((st != 0).sum()) == 0
        say(kernel="witness_schoolbook_verify_kernel", library=os.path.basename(lib_path) if lib_path else "libfrw.so", logn=logn, signatures=k,
            bytes=used, launches=launches, seconds_per_launch=round(t_k, 6), gb_per_s=round(used / t_k / 1e9, 1),
            witnesses_per_s=round(k / t_k, 1), write_stream_seconds=round(t_w, 6), write_stream_gb_per_s=round(used / t_w / 1e9, 1),
            fraction_of_write_stream=round(t_w / t_k, 4))
        del d, inst, st
    eng.close()


def prover_times():
    import torch
    dev = torch.device("cuda:0")
    eng = frw.WitnessEngine(0)
    rng = random.Random(10)
    lim = lambda xs: np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype=np.uint64).reshape(-1, 4)

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, round(time.perf_counter() - t, 4)

    for logn, batch, proof in ((9, 2, True), (10, 1, "--proof1024" in sys.argv)):
        L = frw.layout_schoolbook(logn)
        r, t = wall(lambda: eng.r1cs_load(frw.CIRCUIT_SCHOOLBOOK, logn))
        q = eng.qap_info(r)
        say(call="frw_r1cs_load", circuit="schoolbook", logn=logn, num_witness=L.num_witness, num_constraints=L.num_constraints,
            log_domain_size=int(q.log_domain_size), seconds=t)
        if proof:
            sig, pk, hm = frw.synth_triples(logn, batch, seed=77)
            d = [torch.from_numpy(a.view(np.int16)).to(dev) for a in (sig, pk, hm)]
            wit = torch.empty((batch, L.num_witness, 4), dtype=torch.int64, device=dev)
            inst = torch.empty((batch, L.num_instance, 4), dtype=torch.int64, device=dev)
            st = torch.empty(batch, dtype=torch.int32, device=dev)
            eng.witness_schoolbook_verify_dev(logn, batch, d[0], d[1], d[2], wit, inst, st, frw.ENC_MONTGOMERY, 0)
            (handle, vk), t = wall(lambda: eng.groth16_setup(frw.CIRCUIT_SCHOOLBOOK, logn, *(rng.randrange(2, R) for _ in range(5))))
            say(call="frw_groth16_setup", circuit="schoolbook", logn=logn, seconds=t)
            ws_bytes = eng.groth16_workspace_bytes(handle, r, batch)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            proofs = torch.empty((batch, 48), dtype=torch.int64, device=dev)
            bad = torch.empty(batch, dtype=torch.int32, device=dev)
            rs = np.array([lim([rng.randrange(R), rng.randrange(R)]) for _ in range(batch)])
            for label in ("first call", "second call"):
                _, t = wall(lambda: eng.groth16_prove_dev(handle, r, batch, wit, inst, rs, proofs, ws, ws_bytes, bad, 0))
                say(call="frw_groth16_prove_dev", circuit="schoolbook", logn=logn, proofs=batch, which=label, seconds=t, unsatisfied=bad.tolist())
            ver = frw.Groth16Verifier(vk)
            ok, t = wall(lambda: ver.verify(inst.cpu().numpy().view(np.uint64), proofs.cpu().numpy().view(np.uint64)).tolist())
            say(call="frw_groth16_verify", circuit="schoolbook", logn=logn, accepted=ok, seconds=t)
            ver.close()
            eng.groth16_pk_free(handle)
            del ws, wit, inst
        eng.r1cs_free(r)
    eng.close()


if __name__ == "__main__":
    prover_times() if "--prover" in sys.argv else kernel_rates()
