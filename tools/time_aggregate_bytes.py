"""Time the aggregate prover from bytes on one MI355X (frw_aggregate_prove_from_bytes_dev) against the chain of device calls it
replaces, on the same statements in the same process, alternating; and the stage ahead of the prover by itself.
  statements  the genuine cases of tests/golden/falcon_signed.json, tiled: `9,10,9` (default) or --mix N for N statements alternating
              Falcon-512 / Falcon-1024 (N = 1024: BASELINE configs[4], a key of bare points, 150 GB of device memory)
  chain       per parameter set, on bytes the caller has split by set beforehand: frw_decode_public_keys_dev,
              frw_decode_signatures_dev, frw_hash_to_point_dev, frw_falcon_verify_dev (the screen), frw_witness_ntt_verify_dev; then
              frw_aggregate_assign_dev, frw_groth16_prove_rs_dev, frw_groth16_proofs_to_wire_dev
  one call    frw_aggregate_prove_from_bytes_dev (compressed wire bytes; limbs, instance vector, nonces and count asked for)
  stage       frw_aggregate_falcon_verify_from_bytes_dev alone (routed decoders, SHAKE256, screen, verdicts back in statement order, the
              refused count) and frw_aggregate_statement_from_bytes_dev alone: what runs ahead of the witness kernels
The timed calls are the C entry points with every buffer allocated beforehand; HIP events on one stream around one call (the new call
waits on the host once inside the window, the chain does not).  The two routes' wire bytes must be equal.  --no-prove: the stage only (no
key is made).  One JSON object per line, appended to --out (default profiles/r16_aggregate_bytes.txt).  A record, not a pass mark.
usage: python tools/time_aggregate_bytes.py [reps=5] [--mix N] [--no-prove] [--out PATH]"""
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


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


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
    opts = {"--out": os.path.join(ROOT, "profiles", "r16_aggregate_bytes.txt"), "--mix": None}
    for name in list(opts):
        if name in argv:
            i = argv.index(name)
            opts[name] = argv[i + 1]
            del argv[i:i + 2]
    prove = "--no-prove" not in argv
    argv = [a for a in argv if a != "--no-prove"]
    reps = int(argv[0]) if argv else 5
    logns = [9, 10, 9] if opts["--mix"] is None else [9 + (i & 1) for i in range(int(opts["--mix"]))]
    dev = torch.device("cuda:0")
    eng = frw.WitnessEngine(0)
    lib = frw.load_library()
    with open(os.path.join(ROOT, "tests", "golden", "falcon_signed.json")) as f:
        cases = json.load(f)["cases"]
    pool = {g: [tuple(bytes.fromhex(c[k]) for k in ("pk_bytes", "msg", "sig_bytes")) for c in cases if c["logn"] == g] for g in (9, 10)}
    used, triples = {9: 0, 10: 0}, []
    for g in logns:
        triples.append(pool[g][used[g] % len(pool[g])])
        used[g] += 1
    count = len(triples)
    s0 = torch.cuda.current_stream().cuda_stream
    st = C.c_void_p(s0)
    up = lambda a: torch.from_numpy((a.view(np.int64) if a.dtype == np.uint64 else a).copy()).to(dev)
    handle = eng.r1cs_load_aggregate(logns)
    info = eng.r1cs_info(handle)
    ni, nw = int(info.num_instance), int(info.num_witness)
    _, pkb, sgb, blob, off = eng._aggregate_bytes(triples)
    d_pkb, d_sgb, d_blob, d_off = up(pkb), up(sgb), up(blob), up(off)
    d_non = up(np.frombuffer(b"".join(t[2][1:41] for t in triples), dtype=np.uint8))
    rng = random.Random(16)
    rs = np.frombuffer(b"".join(rng.randrange(R).to_bytes(32, "little") for _ in range(2)), dtype=np.uint64)
    d_rs = up(rs)
    d_status = torch.empty(count, dtype=torch.int32, device=dev)
    d_norm = torch.empty(count, dtype=torch.int64, device=dev)
    d_inst = torch.empty((ni, 4), dtype=torch.int64, device=dev)
    screen_bytes = eng.aggregate_screen_workspace_bytes(handle)
    d_sws = torch.empty(screen_bytes, dtype=torch.uint8, device=dev)

    def stage_screen():
        call(lib.frw_aggregate_falcon_verify_from_bytes_dev(handle, eng._ctx, ptr(d_pkb), ptr(d_sgb), ptr(d_blob), ptr(d_off), 0, ptr(d_status),
                                                            ptr(d_norm), ptr(d_sws), screen_bytes, st))

    def stage_statement():
        call(lib.frw_aggregate_statement_from_bytes_dev(handle, eng._ctx, ptr(d_pkb), ptr(d_non), ptr(d_blob), ptr(d_off), 1, ptr(d_inst),
                                                        ptr(d_status), ptr(d_sws), screen_bytes, st))

    rows = [{"what": "statements", "count": count, "falcon512": logns.count(9), "falcon1024": logns.count(10), "log_domain": int(info.log_domain_size),
             "screen_workspace_bytes": screen_bytes, "reps": reps}]
    stage_screen(); stage_statement()
    torch.cuda.synchronize()
    assert not d_status.any()
    rows.append({"what": "stage: frw_aggregate_falcon_verify_from_bytes_dev", "ms": event_ms(stage_screen, reps)})
    rows.append({"what": "stage: frw_aggregate_statement_from_bytes_dev", "ms": event_ms(stage_statement, reps)})

    if prove:
        key, _ = eng.groth16_setup_r1cs(handle, *(rng.randrange(2, R) for _ in range(5)), want_vk=False)
        # ---- the chain: every buffer of its own, the bytes split by parameter set beforehand
        sets = {}
        for g in (9, 10):
            ts = [t for t in triples if len(t[0]) == frw.PK_LEN[g]]
            if not ts:
                continue
            n, L, c = 1 << g, frw.layout(g), len(ts)
            o = np.zeros(c + 1, dtype=np.uint64)
            o[1:] = np.cumsum([len(t[1]) for t in ts])
            sets[g] = dict(c=c, pkb=up(np.frombuffer(b"".join(t[0] for t in ts), dtype=np.uint8)),
                           sgb=up(np.frombuffer(b"".join(t[2] for t in ts), dtype=np.uint8)),
                           blob=up(np.frombuffer(b"".join(t[1] for t in ts) or b"\0", dtype=np.uint8)), off=up(o),
                           sig=torch.empty((c, n), dtype=torch.int16, device=dev), pk=torch.empty((c, n), dtype=torch.int16, device=dev),
                           hm=torch.empty((c, n), dtype=torch.int16, device=dev), non=torch.empty((c, 40), dtype=torch.uint8, device=dev),
                           st1=torch.empty(c, dtype=torch.int32, device=dev), st2=torch.empty(c, dtype=torch.int32, device=dev),
                           st3=torch.empty(c, dtype=torch.int32, device=dev), st4=torch.empty(c, dtype=torch.int32, device=dev),
                           wit=torch.empty((c, L.num_witness, 4), dtype=torch.int64, device=dev),
                           inst=torch.empty((c, L.num_instance, 4), dtype=torch.int64, device=dev))
        awit = torch.empty((1, nw, 4), dtype=torch.int64, device=dev)
        ainst = torch.empty((1, ni, 4), dtype=torch.int64, device=dev)
        g16_bytes = eng.groth16_workspace_bytes(key, handle, 1)
        d_g16 = torch.empty(g16_bytes, dtype=torch.uint8, device=dev)
        c_proof = torch.empty((1, 48), dtype=torch.int64, device=dev)
        c_bad = torch.empty(1, dtype=torch.int32, device=dev)
        c_wire = torch.empty(192, dtype=torch.uint8, device=dev)
        c_wst = torch.empty(1, dtype=torch.int32, device=dev)

        def chain():
            for g, b in sets.items():
                call(lib.frw_decode_public_keys_dev(eng._ctx, g, b["c"], ptr(b["pkb"]), ptr(b["pk"]), ptr(b["st1"]), st))
                call(lib.frw_decode_signatures_dev(eng._ctx, g, b["c"], ptr(b["sgb"]), frw.SIG_LEN[g], ptr(b["sig"]), ptr(b["non"]), ptr(b["st2"]), st))
                call(lib.frw_hash_to_point_dev(eng._ctx, g, b["c"], ptr(b["non"]), ptr(b["blob"]), ptr(b["off"]), ptr(b["hm"]), st))
                call(lib.frw_falcon_verify_dev(eng._ctx, g, b["c"], ptr(b["sig"]), ptr(b["pk"]), ptr(b["hm"]), 0, ptr(b["st3"]), None, st))
                call(lib.frw_witness_ntt_verify_dev(eng._ctx, g, b["c"], ptr(b["sig"]), ptr(b["pk"]), ptr(b["hm"]), 1, ptr(b["wit"]), ptr(b["inst"]),
                                                    ptr(b["st4"]), st))
            b9, b10 = sets.get(9, {}), sets.get(10, {})
            call(lib.frw_aggregate_assign_dev(handle, ptr(b9.get("wit")), ptr(b9.get("inst")), ptr(b10.get("wit")), ptr(b10.get("inst")), ptr(awit),
                                              ptr(ainst), st))
            call(lib.frw_groth16_prove_rs_dev(key, handle, 1, ptr(awit), ptr(ainst), ptr(d_rs), ptr(c_proof), ptr(c_bad), ptr(d_g16), g16_bytes, st))
            call(lib.frw_groth16_proofs_to_wire_dev(0, 1, ptr(c_proof), 0, ptr(c_wire), ptr(c_wst), st))

        def prover_alone():
            call(lib.frw_groth16_prove_rs_dev(key, handle, 1, ptr(awit), ptr(ainst), ptr(d_rs), ptr(c_proof), ptr(c_bad), ptr(d_g16), g16_bytes, st))

        # ---- the one call
        ws_bytes = eng.aggregate_prove_workspace_bytes(key, handle)
        d_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        o_wire = torch.empty(192, dtype=torch.uint8, device=dev)
        o_proof = torch.empty(48, dtype=torch.int64, device=dev)
        o_non = torch.empty((count, 40), dtype=torch.uint8, device=dev)
        o_bad = torch.empty(1, dtype=torch.int32, device=dev)

        def one_call():
            call(lib.frw_aggregate_prove_from_bytes_dev(eng._ctx, key, handle, ptr(d_pkb), ptr(d_sgb), ptr(d_blob), ptr(d_off), ptr(d_rs), 0,
                                                        ptr(o_wire), ptr(o_proof), ptr(d_inst), ptr(o_non), ptr(d_status), ptr(o_bad), ptr(d_ws),
                                                        ws_bytes, st))

        chain(); one_call()
        torch.cuda.synchronize()
        assert c_bad.tolist() == [0] and o_bad.tolist() == [0] and c_wst.tolist() == [0]
        assert torch.equal(c_wire, o_wire), "the two routes' wire bytes differ"
        rows.append({"what": "workspace", "one_call_bytes": ws_bytes, "groth16_bytes": g16_bytes, "chain_witness_bytes": 2 * 32 * nw})
        a, b = [], []
        for _ in range(2):                                      # alternating
            a.append(event_ms(chain, reps))
            b.append(event_ms(one_call, reps))
        p = event_ms(prover_alone, reps)
        stage = rows[1]["ms"]["median"] + rows[2]["ms"]["median"]
        rows.append({"what": "chain of existing device calls", "ms": a})
        rows.append({"what": "one call: frw_aggregate_prove_from_bytes_dev", "ms": b})
        rows.append({"what": "frw_groth16_prove_rs_dev alone (the proof's time)", "ms": p})
        rows.append({"what": "ratios", "one_call_over_chain": round(b[0]["median"] / a[0]["median"], 4),
                     "stage_over_proof": round(stage / p["median"], 4), "stage_ms": round(stage, 3)})
        eng.groth16_pk_free(key)
    eng.r1cs_free(handle)
    eng.close()
    with open(opts["--out"], "a") as f:
        for r in rows:
            line = json.dumps(r)
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
