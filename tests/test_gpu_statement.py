"""The verifier's statement on the device (statement_kernel in frw_kernels.hip; frw_statement_dev, frw_statement_from_bytes_dev,
frw_aggregate_statement_dev): instance vectors made from (pk, hm) -- or from the key's bytes, the nonce and the message -- without a
signature, held byte for byte to the d_instance the witness entry points write for the same inputs, to the oracle's NTT and codec, and
to the committed digests of the genuine cases; then a proof verified from (pk_bytes, nonce, msg, proof bytes) alone."""
import hashlib
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import frw_testlib as T
from oracle import falcon_codec as FC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = T.Q
P = T.P_FR
R_MONT = (1 << 256) % P
SENTINEL = 0x5A5AA5A53C3CC3C3                        # (fits int64)
NAMES = {0: "ntt", 1: "dual", 2: "schoolbook"}


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).to(torch.device("cuda:0"))


def _expected(oracle, logn, pk, hm, enc, circuit=0):
    """[1, NTT(pk), NTT(hm)] (schoolbook: [1, pk, hm]) of one statement as uint64[2 N + 1, 4]: the oracle's mod-q NTT, lifted into Fr"""
    lift = (lambda p: oracle.ntt_clear(logn, np.asarray(p, dtype=np.uint16))) if circuit != 2 else (lambda p: np.asarray(p))
    vals = [1] + [int(x) for x in lift(pk)] + [int(x) for x in lift(hm)]
    return T.ints_to_limbs([v * R_MONT % P for v in vals] if enc == 1 else vals)


def _witness_instance(engine, circuit, logn, sig, pk, hm, enc):
    """d_instance and the statuses of the matching witness entry point (the parent's only route to an instance vector)"""
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    L = frw.circuit_layout(circuit, logn)
    batch = sig.shape[0]
    wit = torch.empty((batch, L.num_witness, 4), dtype=torch.int64, device=dev)
    inst = torch.empty((batch, L.num_instance, 4), dtype=torch.int64, device=dev)
    st = torch.full((batch,), -1, dtype=torch.int32, device=dev)
    call = (engine.witness_ntt_verify_dev, engine.witness_dual_ntt_verify_dev, engine.witness_schoolbook_verify_dev)[circuit]
    call(logn, batch, _dev(sig), _dev(pk), _dev(hm), wit, inst, st, enc, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    del wit
    return inst, st


def _statement(engine, circuit, logn, pk, hm, enc, guard=64):
    """frw_statement_dev into a buffer with `guard` sentinel elements in front of and behind it -> (instance, status, guards intact)"""
    import torch
    dev = torch.device("cuda:0")
    batch, n = pk.shape
    I = 2 * n + 1
    buf = torch.full(((batch * I + 2 * guard), 4), SENTINEL, dtype=torch.int64, device=dev)
    inst = buf[guard:guard + batch * I].view(batch, I, 4)
    st = torch.full((batch + 2,), -7, dtype=torch.int32, device=dev)
    engine.statement_dev(circuit, logn, batch, _dev(pk), _dev(hm), inst, st[1:], enc, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    intact = bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + batch * I:] == SENTINEL).all()) and int(st[0]) == -7 and int(st[-1]) == -7
    return inst, st[1:1 + batch], intact


# ---- 1. byte equality with the witness kernels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc", [0, 1])
@pytest.mark.parametrize("logn", [9, 10])
@pytest.mark.parametrize("circuit", [0, 1, 2], ids=lambda c: NAMES[c])
def test_instance_equals_the_witness_kernels_byte_for_byte(engine, circuit, logn, enc):
    import torch
    import falcon_r1cs_amd as frw
    batches = (1, 3) if circuit == 2 else (1, 3, 37, 130)          # (a schoolbook witness is 37 MB at logn 10)
    sig, pk, hm = frw.synth_triples(logn, max(batches), seed=900 + 10 * circuit + logn)
    want, want_st = _witness_instance(engine, circuit, logn, sig, pk, hm, enc)
    for batch in batches:
        got, st, intact = _statement(engine, circuit, logn, pk[:batch], hm[:batch], enc)
        assert intact, batch
        assert torch.equal(st, want_st[:batch]) and not st.any(), batch
        assert torch.equal(got, want[:batch]), batch


# ---- 2. edge polynomials ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("circuit,logn,enc", [(0, 9, 1), (0, 10, 0), (2, 9, 0), (2, 10, 1)])
def test_edge_polynomials_in_one_batch(engine, oracle, circuit, logn, enc):
    import falcon_r1cs_amd as frw
    n = 1 << logn
    _, pk, hm = frw.synth_triples(logn, 6, seed=77 + logn)
    pk, hm = pk.copy(), hm.copy()
    pk[0] = 0                                        # all-zero pk
    pk[1] = Q - 1; hm[1] = Q - 1                     # all q - 1
    pk[2] = 0; pk[2, n - 1] = Q - 1                  # a single spike at index N - 1
    pk[3, n - 1] = Q                                 # out of range by one, in the last coefficient
    hm[4, 0] = 0xFFFF                                # out of range, in the first coefficient of the other polynomial
    got, st, intact = _statement(engine, circuit, logn, pk, hm, enc)
    assert intact
    assert st.tolist() == [0, 0, 0, frw.ST_COEFF_RANGE, frw.ST_COEFF_RANGE, 0]
    got = got.cpu().numpy().view(np.uint64)
    for k in (3, 4):
        assert not got[k].any(), k                   # zeros, the leading one included
    for k in (0, 1, 2, 5):
        assert np.array_equal(got[k], _expected(oracle, logn, pk[k], hm[k], enc, circuit)), k


# ---- 3. the stride loop ----------------------------------------------------------------------------------------------------------------
def test_more_statements_than_the_grid_digest_for_digest(engine):
    """4,099 Falcon-512 statements = 8,198 work items: more than any grid the launcher picks (at most four times what the device keeps
    resident, and never more than half the items) and a prime number of statements, so no grid divides them evenly."""
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    logn, batch = 9, 4099
    L = frw.layout(logn)
    s0 = torch.cuda.current_stream().cuda_stream
    sig, pk, hm = frw.synth_triples(logn, batch, seed=4099)
    want_inst = torch.empty((batch, L.num_instance, 4), dtype=torch.int64, device=dev)
    want_st = torch.empty(batch, dtype=torch.int32, device=dev)
    step = 1025                                      # the witness call in four passes: 2.6 GB of witness at a time
    wit = torch.empty((step, L.num_witness, 4), dtype=torch.int64, device=dev)
    for lo in range(0, batch, step):
        cnt = min(step, batch - lo)
        engine.witness_ntt_verify_dev(logn, cnt, _dev(sig[lo:lo + cnt]), _dev(pk[lo:lo + cnt]), _dev(hm[lo:lo + cnt]), wit, want_inst[lo:], want_st[lo:], 1, s0)
    got_inst = torch.full((batch, L.num_instance, 4), SENTINEL, dtype=torch.int64, device=dev)
    got_st = torch.full((batch,), -7, dtype=torch.int32, device=dev)
    engine.statement_dev(0, logn, batch, _dev(pk), _dev(hm), got_inst, got_st, 1, s0)
    dig = torch.zeros((2, batch), dtype=torch.int64, device=dev)
    engine.digest_dev(want_inst, L.num_instance * 4, batch, dig[0], s0)
    engine.digest_dev(got_inst, L.num_instance * 4, batch, dig[1], s0)
    torch.cuda.synchronize()
    assert not want_st.any() and not got_st.any()
    assert torch.equal(dig[0], dig[1])
    assert len(set(dig[1].tolist())) == batch        # (the digests tell the statements apart)


# ---- 4. from bytes ---------------------------------------------------------------------------------------------------------------------
def _cases():
    with open(os.path.join(ROOT, "tests", "golden", "falcon_signed.json")) as f:
        return json.load(f)["cases"]


def test_genuine_cases_from_bytes_equal_the_committed_digests(engine):
    import falcon_r1cs_amd as frw
    cases = _cases()
    assert len(cases) == 4
    for logn in (9, 10):
        sel = [c for c in cases if c["logn"] == logn]
        pkb = [bytes.fromhex(c["pk_bytes"]) for c in sel]
        non = [bytes.fromhex(c["sig_bytes"])[1:41] for c in sel]
        msgs = [bytes.fromhex(c["msg"]) for c in sel]
        d_inst, d_st = engine.statement_from_bytes_dev(0, logn, pkb, non, msgs, frw.ENC_MONTGOMERY)
        inst, st = d_inst.cpu().numpy(), d_st.cpu().numpy()
        assert not st.any()
        for k, c in enumerate(sel):
            assert hashlib.sha256(inst[k].tobytes()).hexdigest() == c["instance_sha256_montgomery"], (logn, k)
        # the host-buffer form gives the same bytes
        h_inst, h_st = engine.statement_from_bytes(0, logn, pkb, non, msgs, frw.ENC_MONTGOMERY)
        assert np.array_equal(h_inst.view(np.int64), inst) and not h_st.any()


@pytest.mark.parametrize("logn", [9, 10])
def test_message_lengths_around_the_shake_rate_and_a_malformed_key(engine, oracle, logn):
    """nonce || msg is 136 bytes, SHAKE256's rate, at a 96-byte message: 95, 96 and 97 straddle the block boundary; 0 is the empty
    message.  The fifth statement's key has a wrong header byte: FRW_ST_DECODE, a zero slot, the neighbours as they should be."""
    import torch
    import falcon_r1cs_amd as frw
    rng = random.Random(136 + logn)
    n = 1 << logn
    lengths = [0, 95, 96, 97, 33, 96]
    pks = [[rng.randrange(Q) for _ in range(n)] for _ in lengths]
    pkb = [FC.modq_encode(p, logn) for p in pks]
    pkb[4] = bytes([pkb[4][0] ^ 0x10]) + pkb[4][1:]
    non = [bytes(rng.randrange(256) for _ in range(40)) for _ in lengths]
    msgs = [bytes(rng.randrange(256) for _ in range(k)) for k in lengths]
    assert [FC.modq_decode(b, logn) is None for b in pkb] == [False, False, False, False, True, False]
    for enc in (0, 1):
        d_inst, d_st = engine.statement_from_bytes_dev(0, logn, pkb, non, msgs, enc)
        torch.cuda.synchronize()
        inst, st = d_inst.cpu().numpy().view(np.uint64), d_st.tolist()
        assert st == [0, 0, 0, 0, frw.ST_DECODE, 0]
        assert not inst[4].any()
        for k in (0, 1, 2, 3, 5):
            assert np.array_equal(inst[k], _expected(oracle, logn, pks[k], FC.hash_to_point(non[k], msgs[k], logn), enc)), (enc, k)
    # strict: FRW_E_RANGE, as everywhere else
    with pytest.raises(frw.FrwError) as ei:
        engine.statement_from_bytes(0, logn, pkb, non, msgs)
    assert ei.value.code == -5
    inst, st = engine.statement_from_bytes(0, logn, pkb, non, msgs, strict=False)
    assert st.tolist() == [0, 0, 0, 0, frw.ST_DECODE, 0] and not inst[4].any()


def test_host_buffer_form_and_strict(engine):
    import falcon_r1cs_amd as frw
    logn = 9
    _, pk, hm = frw.synth_triples(logn, 5, seed=31)
    got, st, _ = _statement(engine, 0, logn, pk, hm, 1)
    inst, hst = engine.statement(0, logn, pk, hm)
    assert np.array_equal(inst.view(np.int64), got.cpu().numpy()) and not hst.any()
    pk = pk.copy()
    pk[2, 7] = Q
    with pytest.raises(frw.FrwError) as ei:
        engine.statement(0, logn, pk, hm)
    assert ei.value.code == -5
    inst, hst = engine.statement(0, logn, pk, hm, strict=False)
    assert hst.tolist() == [0, 0, frw.ST_COEFF_RANGE, 0, 0] and not inst[2].any() and inst[3].any()


# ---- 4b. the host-buffer forms past their first pass ------------------------------------------------------------------------------------
PASS = 4096                                          # statements of one pass of the host-buffer forms (STATEMENT_CHUNK in frw_capi.cpp)


def test_host_form_in_two_passes_equals_the_device_form(engine):
    """4,099 Falcon-512 statements = one full pass and three more.  The device form does not chunk: its instance vectors and statuses
    over the whole batch are the reference, byte for byte.  Statement 4,097 (second pass) has a key coefficient of q."""
    import falcon_r1cs_amd as frw
    logn, batch, bad = 9, PASS + 3, PASS + 1
    _, pk, hm = frw.synth_triples(logn, batch, seed=4099)
    pk = pk.copy()
    pk[bad, 11] = Q
    want, want_st, intact = _statement(engine, 0, logn, pk, hm, 1)
    want, want_st = want.cpu().numpy(), want_st.cpu().numpy()
    assert intact and np.nonzero(want_st)[0].tolist() == [bad] and want_st[bad] == frw.ST_COEFF_RANGE
    inst, st = engine.statement(0, logn, pk, hm, strict=False)
    assert np.array_equal(st, want_st)
    assert np.array_equal(inst.view(np.int64), want)
    assert not inst[bad].any() and inst[bad - 1].any() and inst[bad + 1].any()
    assert not np.array_equal(inst[PASS], inst[0])               # (the second pass is not the first one again)
    with pytest.raises(frw.FrwError) as ei:
        engine.statement(0, logn, pk, hm)
    assert ei.value.code == -5


def test_host_form_from_bytes_in_two_passes_equals_the_device_form(engine):
    """4,099 statements tiled from the two Falcon-512 keys and nonces of the genuine cases with messages of 0, 95, 96, 97, 33, 200 and 13
    bytes (nonce || msg is SHAKE256's rate at 96): a period of 7, which does not divide 4,096, so the second pass's messages differ from
    those at the same positions of the first and their offsets have to be rebased.  Statement 4,097's key has a wrong header byte."""
    import torch
    import falcon_r1cs_amd as frw
    logn, batch, bad = 9, PASS + 3, PASS + 1
    sel = [c for c in _cases() if c["logn"] == logn]
    keys = [bytes.fromhex(c["pk_bytes"]) for c in sel]
    nonces = [bytes.fromhex(c["sig_bytes"])[1:41] for c in sel]
    lengths = [0, 95, 96, 97, 33, 200, 13]
    period = [bytes((5 * i + k) & 255 for i in range(k)) for k in lengths]
    pkb = [keys[(i // 7) % 2] for i in range(batch)]
    non = [nonces[(i // 3) % 2] for i in range(batch)]
    msgs = [period[i % 7] for i in range(batch)]
    assert PASS % 7 and msgs[PASS:PASS + 3] != msgs[:3]
    pkb[bad] = bytes([pkb[bad][0] ^ 0x10]) + pkb[bad][1:]
    d_inst, d_st = engine.statement_from_bytes_dev(0, logn, pkb, non, msgs, frw.ENC_MONTGOMERY)
    torch.cuda.synchronize()
    want, want_st = d_inst.cpu().numpy(), d_st.cpu().numpy()
    assert np.nonzero(want_st)[0].tolist() == [bad] and want_st[bad] == frw.ST_DECODE
    inst, st = engine.statement_from_bytes(0, logn, pkb, non, msgs, frw.ENC_MONTGOMERY, strict=False)
    assert np.array_equal(st, want_st)
    assert np.array_equal(inst.view(np.int64), want)
    assert not inst[bad].any() and inst[bad - 1].any() and inst[bad + 1].any()
    assert not np.array_equal(inst[PASS], inst[0])
    with pytest.raises(frw.FrwError) as ei:
        engine.statement_from_bytes(0, logn, pkb, non, msgs)
    assert ei.value.code == -5


# ---- 5. aggregate ----------------------------------------------------------------------------------------------------------------------
def test_aggregate_statement_equals_aggregate_assign(engine):
    import torch
    import falcon_r1cs_amd as frw
    from test_gpu_aggregate import Aggregate
    dev = torch.device("cuda:0")
    logns = [9, 10, 10, 9, 9]                         # three runs
    agg = Aggregate(engine, logns, seed=611)
    try:
        ni = agg.ni
        assert ni == 7169
        want = agg.inst[0]
        guard = 32

        def run(tr9, tr10):
            buf = torch.full((ni + 2 * guard, 4), SENTINEL, dtype=torch.int64, device=dev)
            st = torch.full((len(logns) + 2,), -7, dtype=torch.int32, device=dev)
            engine.aggregate_statement_dev(agg.handle, _dev(tr9[1]), _dev(tr9[2]), _dev(tr10[1]), _dev(tr10[2]), buf[guard:guard + ni], st[1:], 1, agg.s0)
            torch.cuda.synchronize()
            assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + ni:] == SENTINEL).all())
            assert int(st[0]) == -7 and int(st[-1]) == -7
            return buf[guard:guard + ni], st[1:-1].tolist()

        got, st = run(agg.triples[9], agg.triples[10])
        assert st == [0, 0, 0, 0, 0]
        assert torch.equal(got, want)
        # one hm coefficient >= q in statement 3, the second Falcon-512 one
        sig9, pk9, hm9 = agg.triples[9]
        hm9 = hm9.copy()
        hm9[1, 300] = Q + 5
        got, st = run((sig9, pk9, hm9), agg.triples[10])
        assert st == [0, 0, 0, frw.ST_COEFF_RANGE, 0]
        lo = 1 + 1024 + 2048 + 2048                    # statement 3's 2 N slots
        assert not got[lo:lo + 1024].any()
        assert torch.equal(got[0], want[0])            # the constant is one
        assert torch.equal(got[:lo], want[:lo]) and torch.equal(got[lo + 1024:], want[lo + 1024:])
    finally:
        agg.close()


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------------
def test_a_proof_is_verified_from_key_bytes_nonce_and_message_alone(engine):
    import torch
    import falcon_r1cs_amd as frw
    from test_gpu_verify_dev import R
    dev = torch.device("cuda:0")
    case = _cases()[0]
    logn = case["logn"]
    assert logn == 9
    pk_bytes, msg, sig_bytes = (bytes.fromhex(case[k]) for k in ("pk_bytes", "msg", "sig_bytes"))
    # the prover's side: what the parent could already do
    L = frw.layout(logn)
    sig, pk, hm, st = engine.prepare_inputs(logn, [pk_bytes], [msg], [sig_bytes])
    assert not st.any()
    rng = random.Random(4242)
    key, vk = engine.groth16_setup(0, logn, *(rng.randrange(2, R) for _ in range(5)))
    r1cs = engine.r1cs_load(0, logn)
    try:
        s0 = torch.cuda.current_stream().cuda_stream
        wit = torch.empty((1, L.num_witness, 4), dtype=torch.int64, device=dev)
        inst = torch.empty((1, L.num_instance, 4), dtype=torch.int64, device=dev)
        wst = torch.empty(1, dtype=torch.int32, device=dev)
        engine.witness_ntt_verify_dev(logn, 1, _dev(sig), _dev(pk), _dev(hm), wit, inst, wst, 1, s0)
        ws_bytes = engine.groth16_workspace_bytes(key, r1cs, 1)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        proof = torch.empty((1, 48), dtype=torch.int64, device=dev)
        engine.groth16_prove_dev(key, r1cs, 1, wit, inst, T.ints_to_limbs([rng.randrange(R), rng.randrange(R)]), proof, ws, ws_bytes, None, s0)
        wire, wire_st = frw.proofs_to_wire_dev(proof)
        torch.cuda.synchronize()
        assert int(wst[0]) == 0 and int(wire_st[0]) == 0
        proof_bytes = wire[0].cpu().numpy().tobytes()
        vk_bytes = frw.vk_to_wire(vk)
    finally:
        engine.r1cs_free(r1cs)
        engine.groth16_pk_free(key)
    del wit, inst, ws
    # the verifier's side: the key's bytes, the proof's 192 bytes, the public key, the message, the nonce
    assert len(proof_bytes) == 192
    nonce = sig_bytes[1:41]
    flip = lambda b, i: b[:i] + bytes([b[i] ^ 1]) + b[i + 1:]
    pkbs = [pk_bytes, pk_bytes, pk_bytes, flip(pk_bytes, 0)]
    nons = [nonce, nonce, flip(nonce, 17), nonce]
    msgs = [msg, flip(msg, 3), msg, msg]
    verifier = frw.Groth16Verifier.from_wire(vk_bytes, device=0)
    try:
        status, verdict = verifier.verify_statements_wire_dev(engine, logn, pkbs, nons, msgs, proof_bytes * 4)
        assert status.tolist() == [0, 0, 0, frw.ST_DECODE]
        assert verdict.tolist() == [1, 0, 0, -1]
        seed = np.frombuffer(os.urandom(32), dtype=np.uint64)
        status, verdict = verifier.verify_statements_wire_dev(engine, logn, pkbs, nons, msgs, proof_bytes * 4, batched=True, seed=seed)
        assert status.tolist() == [0, 0, 0, frw.ST_DECODE]
        assert verdict.tolist() == [1, 0, 0, -1]
        status, verdict = verifier.verify_statements_wire_dev(engine, logn, [pk_bytes], [nonce], [msg], proof_bytes, batched=True)
        assert status.tolist() == [0] and verdict.tolist() == [1]
    finally:
        verifier.close()


# ---- 7. the example --------------------------------------------------------------------------------------------------------------------
def test_pok_verify_example_exits_zero():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "pok_verify.py"), os.path.join(ROOT, "tests", "golden", "falcon_signed.json"),
                          "--case", "0"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "verdict 1" in out.stdout and "verdict 0" in out.stdout
