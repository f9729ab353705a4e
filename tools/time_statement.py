"""Time the verifier's statement on one MI355X (frw_statement_dev, frw_statement_from_bytes_dev, Groth16Verifier.verify_statements_wire_dev).
One JSON object per line, also written to --out (default profiles/r11_statement.txt):
  (a) the kernel against the parent's only route to the same bytes: frw_statement_dev for 32,768 Falcon-1024 and 65,536 Falcon-512
      statements -- HIP events around LAUNCHES back-to-back launches on one stream, the launches are well under a millisecond --, next to
      frw_witness_ntt_verify_dev on the same batch (which writes the same instance vectors beside 166 / 164 GB of witness) and to
      frw_diag_write_stream_dev over the statement call's bytes, in the same process, alternating; and the same launch without the
      transform (the schoolbook form), without the Montgomery encode (canonical) and without both: which side binds
  (b) the bytes path: frw_statement_from_bytes_dev (key decoder, SHAKE256, the kernel) for the same batches with 64-byte messages
  (c) verification from the statement's bytes against verification on instance vectors that exist: 4,096 Falcon-1024 proofs (the two
      genuine Falcon-1024 cases of tests/golden/falcon_signed.json, proved once each and tiled) through frw_statement_from_bytes_dev +
      frw_groth16_verify_wire_dev -- what verify_statements_wire_dev runs -- against frw_groth16_verify_wire_dev alone
The timed calls are the C entry points with every buffer allocated beforehand.
usage: python tools/time_statement.py [a|b|c ...] [reps=7] [--out PATH]"""
import ctypes as C
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import falcon_r1cs_amd as frw
import frw_testlib as T

R = T.P_FR
LAUNCHES = 20
SHAPES = ((10, 32768), (9, 65536))
LINES = []


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
    dev = torch.device("cuda:0")
    sig, pk, hm = frw.synth_triples(logn, distinct, seed=11 + logn)
    idx = torch.arange(batch, device=dev) % distinct
    return [torch.from_numpy(a.view(np.int16)).to(dev)[idx].contiguous() for a in (sig, pk, hm)]


def leg_a(eng, lib, reps):
    dev = torch.device("cuda:0")
    s0 = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for logn, batch in SHAPES:
        n = 1 << logn
        L = frw.layout(logn)
        d_sig, d_pk, d_hm = tiled_inputs(logn, batch)
        inst = torch.empty((batch, L.num_instance, 4), dtype=torch.int64, device=dev)
        inst_w = torch.empty((batch, L.num_instance, 4), dtype=torch.int64, device=dev)
        st = torch.empty(batch, dtype=torch.int32, device=dev)
        wit = torch.empty((batch, L.num_witness, 4), dtype=torch.int64, device=dev)
        stream_buf = torch.empty(inst.numel() * 8, dtype=torch.uint8, device=dev)
        out_bytes = inst.numel() * 8

        def statement():
            call(lib.frw_statement_dev(eng._ctx, 0, logn, batch, ptr(d_pk), ptr(d_hm), 1, ptr(inst), ptr(st), s0))

        def witness():
            call(lib.frw_witness_ntt_verify_dev(eng._ctx, logn, batch, ptr(d_sig), ptr(d_pk), ptr(d_hm), 1, ptr(wit), ptr(inst_w), ptr(st), s0))

        def write_stream():
            call(lib.frw_diag_write_stream_dev(eng._ctx, ptr(stream_buf), out_bytes, n * 32, s0))

        # alternating: statement, write stream, witness, and the first two once more (drift shows there)
        t_st = event_ms(statement, reps, LAUNCHES)
        t_ws = event_ms(write_stream, reps, LAUNCHES)
        t_wit = event_ms(witness, max(3, reps // 2))
        torch.cuda.synchronize()
        assert not st.any().item() and torch.equal(inst, inst_w), "the statement call's bytes are not the witness call's"
        t_st2 = event_ms(statement, reps, LAUNCHES)
        t_ws2 = event_ms(write_stream, reps, LAUNCHES)
        t_one = event_ms(statement, reps, 1)
        # which side binds: the same launch without the transform (the schoolbook form), without the Montgomery encode (canonical), without both
        variant = lambda circuit, enc: event_ms(lambda: call(lib.frw_statement_dev(eng._ctx, circuit, logn, batch, ptr(d_pk), ptr(d_hm), enc, ptr(inst),
                                                                                   ptr(st), s0)), reps, LAUNCHES)
        t_noxf, t_noenc, t_bare = variant(2, 1), variant(0, 0), variant(2, 0)
        emit({"case": "a: frw_statement_dev, %d Falcon-%d statements" % (batch, n), "batch": batch, "logn": logn, "reps": reps,
              "launches_per_event_pair": LAUNCHES, "instance_bytes": out_bytes, "witness_call_bytes": int(wit.numel() * 8 + out_bytes),
              "statement_ms": ms(t_st), "statement_again_ms": ms(t_st2), "statement_single_launch_ms": ms(t_one),
              "statement_GBps": round(out_bytes / t_st[0] / 1e6, 1), "statements_per_s": round(batch / t_st[0] * 1e3, 0),
              "write_stream_same_bytes_ms": ms(t_ws), "write_stream_again_ms": ms(t_ws2), "write_stream_GBps": round(out_bytes / t_ws[0] / 1e6, 1),
              "statement_over_write_stream": round(t_st[0] / t_ws[0], 3),
              "no_transform_ms": ms(t_noxf), "no_encode_ms": ms(t_noenc), "no_transform_no_encode_ms": ms(t_bare),
              "witness_ntt_verify_ms": ms(t_wit), "witness_GBps": round((wit.numel() * 8 + out_bytes) / t_wit[0] / 1e6, 1),
              "statement_over_witness": round(t_st[0] / t_wit[0], 5)})
        del wit, inst, inst_w, stream_buf
        torch.cuda.empty_cache()


def random_bytes_inputs(logn, batch, msg_len, distinct=4096):
    """well-formed keys (14-bit coefficients below q), nonces and messages: `distinct` of them, tiled on the device"""
    dev = torch.device("cuda:0")
    n = 1 << logn
    rng = np.random.default_rng(logn)
    coeffs = rng.integers(0, T.Q, (distinct, n), dtype=np.uint64)
    bits = ((coeffs[:, :, None] >> np.arange(13, -1, -1, dtype=np.uint64)) & 1).astype(np.uint8).reshape(distinct, 14 * n)
    pkb = np.concatenate([np.full((distinct, 1), logn, dtype=np.uint8), np.packbits(bits, axis=1)], axis=1)
    assert pkb.shape[1] == frw.PK_LEN[logn]
    idx = torch.arange(batch, device=dev) % distinct
    d_pkb = torch.from_numpy(pkb).to(dev)[idx].contiguous()
    d_non = torch.from_numpy(rng.integers(0, 256, (distinct, 40), dtype=np.uint8)).to(dev)[idx].contiguous()
    d_msgs = torch.from_numpy(rng.integers(0, 256, (distinct, msg_len), dtype=np.uint8)).to(dev)[idx].contiguous()
    d_off = (torch.arange(batch + 1, dtype=torch.int64, device=dev) * msg_len).contiguous()
    return d_pkb, d_non, d_msgs, d_off


def leg_b(eng, lib, reps, msg_len=64):
    dev = torch.device("cuda:0")
    s0 = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for logn, batch in SHAPES:
        n = 1 << logn
        d_pkb, d_non, d_msgs, d_off = random_bytes_inputs(logn, batch, msg_len)
        inst = torch.empty((batch, 2 * n + 1, 4), dtype=torch.int64, device=dev)
        st = torch.empty(batch, dtype=torch.int32, device=dev)
        ws = torch.empty(eng.statement_workspace_bytes(logn, batch), dtype=torch.uint8, device=dev)
        pk = torch.empty((batch, n), dtype=torch.int16, device=dev)
        hm = torch.empty((batch, n), dtype=torch.int16, device=dev)

        def chain():
            call(lib.frw_statement_from_bytes_dev(eng._ctx, 0, logn, batch, ptr(d_pkb), ptr(d_non), ptr(d_msgs), ptr(d_off), 1, ptr(inst), ptr(st),
                                                  ptr(ws), ws.numel(), s0))

        t_chain = event_ms(chain, reps, 5)
        torch.cuda.synchronize()
        assert not st.any().item()
        t_dec = event_ms(lambda: call(lib.frw_decode_public_keys_dev(eng._ctx, logn, batch, ptr(d_pkb), ptr(pk), ptr(st), s0)), reps, 5)
        t_hash = event_ms(lambda: call(lib.frw_hash_to_point_dev(eng._ctx, logn, batch, ptr(d_non), ptr(d_msgs), ptr(d_off), ptr(hm), s0)), reps, 5)
        t_st = event_ms(lambda: call(lib.frw_statement_dev(eng._ctx, 0, logn, batch, ptr(pk), ptr(hm), 1, ptr(inst), ptr(st), s0)), reps, LAUNCHES)
        emit({"case": "b: frw_statement_from_bytes_dev, %d Falcon-%d statements, %d-byte messages" % (batch, n, msg_len), "batch": batch, "logn": logn,
              "reps": reps, "from_bytes_ms": ms(t_chain), "statements_per_s": round(batch / t_chain[0] * 1e3, 0),
              "decode_public_keys_ms": ms(t_dec), "hash_to_point_ms": ms(t_hash), "statement_kernel_ms": ms(t_st),
              "workspace_bytes": int(ws.numel())})
        del inst, ws, pk, hm
        torch.cuda.empty_cache()


def leg_c(eng, lib, reps, n_proofs=4096, logn=10):
    dev = torch.device("cuda:0")
    s0 = torch.cuda.current_stream().cuda_stream
    with open(os.path.join(ROOT, "tests", "golden", "falcon_signed.json")) as f:
        cases = [c for c in json.load(f)["cases"] if c["logn"] == logn]
    pkb, msgs, sigb = ([bytes.fromhex(c[k]) for c in cases] for k in ("pk_bytes", "msg", "sig_bytes"))
    k = len(cases)
    L = frw.layout(logn)
    sig, pk, hm, st = eng.prepare_inputs(logn, pkb, msgs, sigb)
    assert not st.any()
    rng = random.Random(5)
    key, vk = eng.groth16_setup(0, logn, *(rng.randrange(2, R) for _ in range(5)))
    r1cs = eng.r1cs_load(0, logn)
    d = [torch.from_numpy(a.view(np.int16)).to(dev) for a in (sig, pk, hm)]
    wit = torch.empty((k, L.num_witness, 4), dtype=torch.int64, device=dev)
    inst = torch.empty((k, L.num_instance, 4), dtype=torch.int64, device=dev)
    wst = torch.empty(k, dtype=torch.int32, device=dev)
    eng.witness_ntt_verify_dev(logn, k, d[0], d[1], d[2], wit, inst, wst, 1, s0)
    ws_bytes = eng.groth16_workspace_bytes(key, r1cs, k)
    pws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    proofs = torch.empty((k, 48), dtype=torch.int64, device=dev)
    eng.groth16_prove_dev(key, r1cs, k, wit, inst, np.array([T.ints_to_limbs([rng.randrange(R), rng.randrange(R)]) for _ in range(k)]), proofs, pws,
                          ws_bytes, None, s0)
    wire, wire_st = frw.proofs_to_wire_dev(proofs)
    torch.cuda.synchronize()
    assert not wst.any().item() and not wire_st.any().item()
    del wit, pws
    eng.r1cs_free(r1cs)
    eng.groth16_pk_free(key)
    ver = frw.Groth16Verifier.from_wire(frw.vk_to_wire(vk), device=0)
    # the batch: the k genuine statements, tiled
    idx = torch.arange(n_proofs, device=dev) % k
    d_inst, d_wire = inst[idx].contiguous(), wire[idx].contiguous()
    up = lambda blob: torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(dev)
    d_pkb = up(b"".join(pkb)).view(k, -1)[idx].contiguous()
    d_non = up(b"".join(s[1:41] for s in sigb)).view(k, 40)[idx].contiguous()
    lens = [len(msgs[i % k]) for i in range(n_proofs)]
    d_msgs = up(b"".join(msgs[i % k] for i in range(n_proofs)) or b"\0")
    d_off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)
    made = torch.empty_like(d_inst)
    sst = torch.empty(n_proofs, dtype=torch.int32, device=dev)
    sws = torch.empty(eng.statement_workspace_bytes(logn, n_proofs), dtype=torch.uint8, device=dev)
    vws = torch.empty(ver.wire_workspace_bytes(n_proofs, 0, True), dtype=torch.uint8, device=dev)
    verdicts = torch.empty(n_proofs, dtype=torch.int32, device=dev)
    cs = C.c_void_p(s0)

    def statement():
        call(lib.frw_statement_from_bytes_dev(eng._ctx, 0, logn, n_proofs, ptr(d_pkb), ptr(d_non), ptr(d_msgs), ptr(d_off), 1, ptr(made), ptr(sst),
                                              ptr(sws), sws.numel(), cs))

    def verify(which):
        call(lib.frw_groth16_verify_wire_dev(ver._h, n_proofs, ptr(which), 1, ptr(d_wire), 0, 0, None, ptr(verdicts), None, ptr(vws), vws.numel(), cs))

    def from_bytes():
        statement()
        verify(made)

    t_given = event_ms(lambda: verify(d_inst), reps)
    assert int((verdicts == 1).sum()) == n_proofs
    verdicts.zero_()
    t_bytes = event_ms(from_bytes, reps)
    assert int((verdicts == 1).sum()) == n_proofs and not sst.any().item() and torch.equal(made, d_inst)
    t_given2 = event_ms(lambda: verify(d_inst), reps)
    t_stmt = event_ms(statement, reps, 5)
    # the Python face once, for the verdicts (it allocates and uploads: not what is timed above)
    status, got = ver.verify_statements_wire_dev(eng, logn, pkb, [s[1:41] for s in sigb], msgs, wire)
    assert status.tolist() == [0] * k and got.tolist() == [1] * k
    emit({"case": "c: %d Falcon-1024 proofs, verification from (pk_bytes, nonce, msg, proof bytes)" % n_proofs, "batch": n_proofs, "reps": reps,
          "verify_wire_dev_given_instance_ms": ms(t_given), "verify_wire_dev_given_instance_again_ms": ms(t_given2),
          "statement_from_bytes_then_verify_wire_dev_ms": ms(t_bytes), "statement_from_bytes_alone_ms": ms(t_stmt),
          "from_bytes_over_given_instance": round(t_bytes[0] / t_given[0], 4),
          "proofs_per_s_given_instance": round(n_proofs / t_given[0] * 1e3, 0), "proofs_per_s_from_bytes": round(n_proofs / t_bytes[0] * 1e3, 0)})
    ver.close()


def main():
    argv = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "r11_statement.txt")
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    legs = [a for a in argv if not a.isdigit()] or ["a", "b", "c"]
    reps = int(next((a for a in argv if a.isdigit()), 7))
    eng = frw.WitnessEngine(0)
    lib = frw.load_library()
    emit({"tool": "tools/time_statement.py", "device": torch.cuda.get_device_name(0), "reps": reps,
          "timed": "C entry points, buffers allocated beforehand, HIP events on one stream; ms per call"})
    for leg in legs:
        {"a": leg_a, "b": leg_b, "c": leg_c}[leg](eng, lib, reps)
        torch.cuda.empty_cache()
    eng.close()
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
