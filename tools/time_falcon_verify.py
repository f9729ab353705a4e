"""Time Falcon verification without a witness on one MI355X (frw_falcon_verify_dev, frw_falcon_verify_from_bytes_dev).  One JSON object
per line, also written to --out (default profiles/r12_falcon_verify.txt):
  (a) the kernel against the two existing routes to the same status words, on the same batch, in the same process, alternating:
      frw_falcon_verify_dev (HIP events around LAUNCHES back-to-back launches: a launch is well under a millisecond),
      frw_witness_ntt_verify_compact_dev (the cheapest of them) and frw_witness_ntt_verify_dev; 32,768 Falcon-1024 and 65,536 Falcon-512
      signatures.  The statuses of the three must be equal.  THE ONE CONDITION: the kernel's median below the compact call's -- the tool
      exits 1 otherwise.
  (b) the bytes path: frw_falcon_verify_from_bytes_dev with 64-byte messages (genuine signatures made here with oracle/falcon_sign.py
      from the fixture's key seeds, tiled) against its four kernels apart: which stage binds
  (c) what the kernel's time is made of: other builds of the library, given as --variant NAME=PATH, timed on (a)'s batch alternating
      with this build.  frw_kernels.hip compiled with -DFRW_FV_STAGE=1 leaves the inverse transform out, -DFRW_FV_STAGE=2 everything but
      the loads, the range check and the norm.  (The recorded run also has a build whose kernel copied the inverse twiddles to LDS
      instead of reading the table: 0.966 / 0.982 of this build, not taken.)
The timed calls are the C entry points with every buffer allocated beforehand.
usage: python tools/time_falcon_verify.py [a|b|c ...] [reps=7] [--out PATH] [--variant NAME=PATH ...]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import falcon_r1cs_amd as frw

LAUNCHES = 20
SHAPES = ((10, 32768), (9, 65536))
LINES = []
FAILED = []


def emit(obj):
    line = json.dumps(obj)
    LINES.append(line)
    print(line, flush=True)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def call(rc):
    if rc:
        raise RuntimeError("frw call failed: %d (%s)" % (rc, frw.load_library().frw_last_error().decode()))


def event_ms(fn, reps, launches=1):
    """ms per call of fn() from HIP events around `launches` back-to-back calls on the current stream: (median, min) over `reps`"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / launches)
    return sorted(times)[len(times) // 2], min(times)


def ms(pair):
    return {"median": round(pair[0], 4), "min": round(pair[1], 4)}


def tiled_inputs(logn, batch, distinct=4096):
    """valid triples, every 64th one's hm replaced (FRW_ST_NORM_BOUND), tiled on the device"""
    dev = torch.device("cuda:0")
    sig, pk, hm = (a.copy() for a in frw.synth_triples(logn, distinct, seed=11 + logn))
    hm[0::64] = np.random.default_rng(logn).integers(0, 12289, (distinct // 64, 1 << logn), dtype=np.uint16)
    idx = torch.arange(batch, device=dev) % distinct
    return [torch.from_numpy(a.view(np.int16)).to(dev)[idx].contiguous() for a in (sig, pk, hm)]


def other_build(path):
    """(library, context) of another build of libfrw.so, with the entry point timed here"""
    lib = C.CDLL(os.path.abspath(path))
    lib.frw_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.frw_falcon_verify_dev.argtypes = frw._lib.PROTOTYPES["frw_falcon_verify_dev"][1]
    ctx = C.c_void_p()
    assert lib.frw_ctx_create(0, C.byref(ctx)) == 0
    return lib, ctx


def leg_a(eng, lib, reps, variants):
    dev = torch.device("cuda:0")
    s0 = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for logn, batch in SHAPES:
        n = 1 << logn
        L = frw.layout(logn)
        CL = frw.compact_layout(logn)
        d_sig, d_pk, d_hm = tiled_inputs(logn, batch)
        st, st_c, st_w = (torch.full((batch,), -7, dtype=torch.int32, device=dev) for _ in range(3))
        norm = torch.empty(batch, dtype=torch.int64, device=dev)
        compact = torch.empty(batch * CL.bytes_per_signature, dtype=torch.uint8, device=dev)
        wit = torch.empty((batch, L.num_witness, 4), dtype=torch.int64, device=dev)
        inst = torch.empty((batch, L.num_instance, 4), dtype=torch.int64, device=dev)

        def verify(rule=0, d_norm=norm, which=(lib, eng._ctx), out=st):
            call(which[0].frw_falcon_verify_dev(which[1], logn, batch, ptr(d_sig), ptr(d_pk), ptr(d_hm), rule, ptr(out),
                                                ptr(d_norm) if d_norm is not None else None, s0))

        def compact_call():
            call(lib.frw_witness_ntt_verify_compact_dev(eng._ctx, logn, batch, ptr(d_sig), ptr(d_pk), ptr(d_hm), ptr(compact), ptr(st_c), s0))

        def witness():
            call(lib.frw_witness_ntt_verify_dev(eng._ctx, logn, batch, ptr(d_sig), ptr(d_pk), ptr(d_hm), 1, ptr(wit), ptr(inst), ptr(st_w), s0))

        # alternating: verify, compact, witness, and the first two once more (drift shows there)
        t_v = event_ms(verify, reps, LAUNCHES)
        t_c = event_ms(compact_call, reps)
        t_w = event_ms(witness, max(3, reps // 2))
        torch.cuda.synchronize()
        assert torch.equal(st, st_c) and torch.equal(st, st_w), "the verdicts are not the witness calls' status words"
        refused = int((st != 0).sum())
        assert refused == batch // 64
        t_v2 = event_ms(verify, reps, LAUNCHES)
        t_c2 = event_ms(compact_call, reps)
        t_one = event_ms(verify, reps, 1)
        t_spec = event_ms(lambda: verify(rule=1), reps, LAUNCHES)
        t_nonorm = event_ms(lambda: verify(d_norm=None), reps, LAUNCHES)
        row = {"case": "a: frw_falcon_verify_dev, %d Falcon-%d signatures" % (batch, n), "batch": batch, "logn": logn, "reps": reps,
               "launches_per_event_pair": LAUNCHES, "refused": refused, "input_bytes": 3 * batch * n * 2, "output_bytes": 12 * batch,
               "compact_call_bytes": int(compact.numel()), "witness_call_bytes": int(wit.numel() * 8 + inst.numel() * 8),
               "verify_ms": ms(t_v), "verify_again_ms": ms(t_v2), "verify_single_launch_ms": ms(t_one), "verify_rule_spec_ms": ms(t_spec),
               "verify_without_norm_ms": ms(t_nonorm), "signatures_per_s": round(batch / t_v[0] * 1e3, 0),
               "input_GBps": round(3 * batch * n * 2 / t_v[0] / 1e6, 1),
               "witness_compact_ms": ms(t_c), "witness_compact_again_ms": ms(t_c2), "witness_ntt_verify_ms": ms(t_w),
               "verify_over_compact": round(t_v[0] / t_c[0], 5), "verify_over_witness": round(t_v[0] / t_w[0], 5)}
        del wit, inst, compact
        torch.cuda.empty_cache()
        # (c) on the same batch: each other build alternating with this one
        for name, (vlib, vctx) in variants.items():
            other = torch.full((batch,), -7, dtype=torch.int32, device=dev)
            t_x = event_ms(lambda: verify(which=(vlib, vctx), out=other), reps, LAUNCHES)
            t_m = event_ms(verify, reps, LAUNCHES)
            row["c: %s_ms" % name] = ms(t_x)
            row["c: this_build_next_to_%s_ms" % name] = ms(t_m)
            row["c: %s_over_this_build" % name] = round(t_x[0] / t_m[0], 4)
            row["c: %s_same_statuses" % name] = bool(torch.equal(other, st))
        emit(row)
        if not t_v[0] < t_c[0]:
            FAILED.append("Falcon-%d: frw_falcon_verify_dev %.4f ms is not below the compact witness call's %.4f ms" % (n, t_v[0], t_c[0]))


def signed_bytes_inputs(logn, batch, msg_len=64, distinct=4):
    """genuine (pk, sig, msg) with `msg_len`-byte messages: the fixture's first key of this logn (oracle/falcon_sign.py, from its seed)
    signs `distinct` messages; tiled on the device"""
    from oracle import falcon_sign as S
    dev = torch.device("cuda:0")
    with open(os.path.join(ROOT, "tests", "golden", "falcon_signed.json")) as f:
        case = [c for c in json.load(f)["cases"] if c["logn"] == logn][0]
    seed = bytes.fromhex(case["key_seed"])
    sk = S.keygen(logn, seed)
    pkb = sk.public_key_bytes()
    msgs = [bytes((k * 37 + i) & 255 for i in range(msg_len)) for k in range(distinct)]
    sigs = [S.sign(sk, m, seed + bytes([k])) for k, m in enumerate(msgs)]
    assert all(S.verify(pkb, m, s, logn) for m, s in zip(msgs, sigs))
    up = lambda blob, w: torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(dev).view(-1, w)
    idx = torch.arange(batch, device=dev) % distinct
    d_pkb = up(pkb * distinct, len(pkb))[idx].contiguous()
    d_sgb = up(b"".join(sigs), len(sigs[0]))[idx].contiguous()
    d_msgs = up(b"".join(msgs), msg_len)[idx].contiguous()
    d_off = (torch.arange(batch + 1, dtype=torch.int64, device=dev) * msg_len).contiguous()
    return d_pkb, d_sgb, len(sigs[0]), d_msgs, d_off


def leg_b(eng, lib, reps, msg_len=64):
    dev = torch.device("cuda:0")
    s0 = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for logn, batch in SHAPES:
        n = 1 << logn
        d_pkb, d_sgb, sig_len, d_msgs, d_off = signed_bytes_inputs(logn, batch, msg_len)
        st = torch.full((batch,), -7, dtype=torch.int32, device=dev)
        st2 = torch.empty(batch, dtype=torch.int32, device=dev)
        norm = torch.empty(batch, dtype=torch.int64, device=dev)
        ws = torch.empty(eng.falcon_verify_workspace_bytes(logn, batch), dtype=torch.uint8, device=dev)
        sig, pk, hm = (torch.empty((batch, n), dtype=torch.int16, device=dev) for _ in range(3))
        nonce = torch.empty((batch, 40), dtype=torch.uint8, device=dev)

        def chain():
            call(lib.frw_falcon_verify_from_bytes_dev(eng._ctx, logn, batch, ptr(d_pkb), ptr(d_sgb), sig_len, ptr(d_msgs), ptr(d_off), 0, ptr(st),
                                                      ptr(norm), ptr(ws), ws.numel(), s0))

        t_chain = event_ms(chain, reps, 5)
        torch.cuda.synchronize()
        assert not st.any().item(), "a genuine signature was refused"
        t_dpk = event_ms(lambda: call(lib.frw_decode_public_keys_dev(eng._ctx, logn, batch, ptr(d_pkb), ptr(pk), ptr(st2), s0)), reps, 5)
        t_dsg = event_ms(lambda: call(lib.frw_decode_signatures_dev(eng._ctx, logn, batch, ptr(d_sgb), sig_len, ptr(sig), ptr(nonce), ptr(st2), s0)), reps, 5)
        t_hash = event_ms(lambda: call(lib.frw_hash_to_point_dev(eng._ctx, logn, batch, ptr(nonce), ptr(d_msgs), ptr(d_off), ptr(hm), s0)), reps, 5)
        t_k = event_ms(lambda: call(lib.frw_falcon_verify_dev(eng._ctx, logn, batch, ptr(sig), ptr(pk), ptr(hm), 0, ptr(st2), ptr(norm), s0)), reps, LAUNCHES)
        torch.cuda.synchronize()
        assert not st2.any().item()
        t_chain2 = event_ms(chain, reps, 5)
        parts = t_dpk[0] + t_dsg[0] + t_hash[0] + t_k[0]
        emit({"case": "b: frw_falcon_verify_from_bytes_dev, %d Falcon-%d signatures, %d-byte messages" % (batch, n, msg_len), "batch": batch,
              "logn": logn, "reps": reps, "sig_len": sig_len, "from_bytes_ms": ms(t_chain), "from_bytes_again_ms": ms(t_chain2),
              "signatures_per_s": round(batch / t_chain[0] * 1e3, 0), "decode_public_keys_ms": ms(t_dpk), "decode_signatures_ms": ms(t_dsg),
              "hash_to_point_ms": ms(t_hash), "verify_kernel_ms": ms(t_k), "sum_of_the_four_ms": round(parts, 4),
              "share_of_the_sum": {"decode_public_keys": round(t_dpk[0] / parts, 3), "decode_signatures": round(t_dsg[0] / parts, 3),
                                   "hash_to_point": round(t_hash[0] / parts, 3), "verify_kernel": round(t_k[0] / parts, 3)},
              "workspace_bytes": int(ws.numel())})
        del ws, sig, pk, hm
        torch.cuda.empty_cache()


def main():
    argv = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "r12_falcon_verify.txt")
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    variant_paths = {}
    while "--variant" in argv:
        i = argv.index("--variant")
        name, path = argv[i + 1].split("=", 1)
        variant_paths[name] = path
        del argv[i:i + 2]
    legs = [a for a in argv if not a.isdigit()] or ["a", "b"]
    reps = int(next((a for a in argv if a.isdigit()), 7))
    eng = frw.WitnessEngine(0)
    lib = frw.load_library()
    variants = {name: other_build(path) for name, path in variant_paths.items()} if ("a" in legs or "c" in legs) else {}
    emit({"tool": "tools/time_falcon_verify.py", "device": torch.cuda.get_device_name(0), "reps": reps, "variants": sorted(variant_paths),
          "timed": "C entry points, buffers allocated beforehand, HIP events on one stream; ms per call"})
    if "a" in legs or "c" in legs:
        leg_a(eng, lib, reps, variants)
        torch.cuda.empty_cache()
    if "b" in legs:
        leg_b(eng, lib, reps)
    eng.close()
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    if FAILED:
        raise SystemExit("; ".join(FAILED))


if __name__ == "__main__":
    main()
