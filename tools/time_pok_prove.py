"""Time the prover from bytes on one MI355X (frw_pok_prove_from_bytes_dev) against the chain of device calls it replaces, on the same
batch in the same process, alternating: 64 Falcon-1024 signatures, all accepted (the two genuine Falcon-1024 cases of
tests/golden/falcon_signed.json, tiled), 64 proofs in flight for both.
  chain     frw_decode_public_keys_dev, frw_decode_signatures_dev, frw_hash_to_point_dev, frw_falcon_verify_dev (the screen),
            frw_witness_ntt_verify_dev, frw_groth16_prove_rs_dev, frw_groth16_proofs_to_wire_dev
  one call  frw_pok_prove_from_bytes_dev (compressed wire bytes; limbs, instance vectors and counts asked for)
The timed calls are the C entry points with every buffer allocated beforehand; HIP events on one stream around one call (the new call
waits on the host once inside the window, the chain does not).  The two routes' wire bytes must be equal.  One JSON object per line, also
written to --out (default profiles/r13_pok_prove.txt).  A record, not a pass mark: the prover's time dominates both and is unchanged.
usage: python tools/time_pok_prove.py [reps=5] [--out PATH]"""
import ctypes as C
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import falcon_r1cs_amd as frw

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
LOGN, BATCH = 10, 64


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


def main():
    argv = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "r13_pok_prove.txt")
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    reps = int(argv[0]) if argv else 5
    dev = torch.device("cuda:0")
    eng = frw.WitnessEngine(0)
    lib = frw.load_library()
    with open(os.path.join(ROOT, "tests", "golden", "falcon_signed.json")) as f:
        cases = [c for c in json.load(f)["cases"] if c["logn"] == LOGN]
    triples = [tuple(bytes.fromhex(cases[i % len(cases)][k]) for k in ("pk_bytes", "msg", "sig_bytes")) for i in range(BATCH)]
    up = lambda blob: torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(dev)
    d_pkb, d_msgs, d_sgb = (up(b"".join(t[k] for t in triples)) for k in range(3))
    d_off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(t[1]) for t in triples])]).astype(np.int64)).to(dev)
    rng = random.Random(13)
    key, _ = eng.groth16_setup(frw.CIRCUIT_NTT, LOGN, *(rng.randrange(2, R) for _ in range(5)))
    r1cs = eng.r1cs_load(frw.CIRCUIT_NTT, LOGN)
    rs = np.frombuffer(b"".join(rng.randrange(R).to_bytes(32, "little") for _ in range(2 * BATCH)), dtype=np.int64).copy()
    d_rs = torch.from_numpy(rs).to(dev)
    L = frw.layout(LOGN)
    n, sig_len = L.n, frw.SIG_LEN[LOGN]
    s0 = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    i16 = lambda: torch.empty((BATCH, n), dtype=torch.int16, device=dev)
    i32 = lambda: torch.empty(BATCH, dtype=torch.int32, device=dev)
    # the chain's buffers
    sig, pk, hm, nonce = i16(), i16(), i16(), torch.empty((BATCH, 40), dtype=torch.uint8, device=dev)
    st_pk, st_sig, st, wst, bad, wire_st = i32(), i32(), i32(), i32(), i32(), i32()
    wit = torch.empty((BATCH, L.num_witness, 4), dtype=torch.int64, device=dev)
    inst = torch.empty((BATCH, L.num_instance, 4), dtype=torch.int64, device=dev)
    proofs = torch.empty((BATCH, 48), dtype=torch.int64, device=dev)
    wire = torch.zeros((BATCH, 192), dtype=torch.uint8, device=dev)
    gws = torch.empty(eng.groth16_workspace_bytes(key, r1cs, BATCH), dtype=torch.uint8, device=dev)
    # the one call's
    ws = torch.empty(eng.pok_prove_workspace_bytes(key, r1cs, frw.CIRCUIT_NTT, LOGN, BATCH, BATCH), dtype=torch.uint8, device=dev)
    wire2 = torch.zeros((BATCH, 192), dtype=torch.uint8, device=dev)
    proofs2, inst2, st2, bad2 = torch.empty_like(proofs), torch.empty_like(inst), i32(), i32()

    def chain():
        call(lib.frw_decode_public_keys_dev(eng._ctx, LOGN, BATCH, ptr(d_pkb), ptr(pk), ptr(st_pk), s0))
        call(lib.frw_decode_signatures_dev(eng._ctx, LOGN, BATCH, ptr(d_sgb), sig_len, ptr(sig), ptr(nonce), ptr(st_sig), s0))
        call(lib.frw_hash_to_point_dev(eng._ctx, LOGN, BATCH, ptr(nonce), ptr(d_msgs), ptr(d_off), ptr(hm), s0))
        call(lib.frw_falcon_verify_dev(eng._ctx, LOGN, BATCH, ptr(sig), ptr(pk), ptr(hm), 0, ptr(st), None, s0))
        call(lib.frw_witness_ntt_verify_dev(eng._ctx, LOGN, BATCH, ptr(sig), ptr(pk), ptr(hm), 1, ptr(wit), ptr(inst), ptr(wst), s0))
        call(lib.frw_groth16_prove_rs_dev(key, r1cs, BATCH, ptr(wit), ptr(inst), ptr(d_rs), ptr(proofs), ptr(bad), ptr(gws), gws.numel(), s0))
        call(lib.frw_groth16_proofs_to_wire_dev(0, BATCH, ptr(proofs), 0, ptr(wire), ptr(wire_st), s0))

    def one_call():
        call(lib.frw_pok_prove_from_bytes_dev(eng._ctx, key, r1cs, frw.CIRCUIT_NTT, LOGN, BATCH, ptr(d_pkb), ptr(d_sgb), sig_len, ptr(d_msgs),
                                              ptr(d_off), ptr(d_rs), 0, ptr(wire2), ptr(proofs2), ptr(inst2), ptr(st2), ptr(bad2), ptr(ws),
                                              ws.numel(), s0))

    for _ in range(2):
        chain()
        one_call()
    torch.cuda.synchronize()
    assert not st.any().item() and not st2.any().item() and not bad.any().item() and not bad2.any().item()
    assert torch.equal(wire, wire2) and torch.equal(proofs, proofs2) and torch.equal(inst, inst2), "the two routes' bytes differ"
    t = [event_ms(chain, reps), event_ms(one_call, reps), event_ms(chain, reps), event_ms(one_call, reps)]
    lines = [json.dumps({"tool": "tools/time_pok_prove.py", "device": torch.cuda.get_device_name(0), "reps": reps,
                         "timed": "C entry points, buffers allocated beforehand, HIP events on one stream around one call; ms per call"}),
             json.dumps({"case": "%d Falcon-%d signatures, all accepted, %d proofs in flight" % (BATCH, n, BATCH), "chain_ms": t[0],
                         "one_call_ms": t[1], "chain_again_ms": t[2], "one_call_again_ms": t[3],
                         "one_call_over_chain": round(t[1]["median"] / t[0]["median"], 4), "bytes_equal": True,
                         "workspace_bytes": int(ws.numel()), "chain_witness_plus_prover_workspace_bytes": int(wit.numel() * 8 + gws.numel())})]
    print("\n".join(lines), flush=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    eng.r1cs_free(r1cs)
    eng.groth16_pk_free(key)
    eng.close()


if __name__ == "__main__":
    main()
