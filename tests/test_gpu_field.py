"""Witness bytes over any four-limb scalar field (the ENC = 3 instantiations of frw_kernels.hip behind frw_ctx_field_encoding):
  1. parity with the arkworks front-end simulation run over that field (oracle/ark_sim.ConstraintSystem(p) + oracle/falcon_gadgets),
     element by element as value * 2^256 mod p, the oracle's system satisfied;
  2. with BLS12-381's own modulus registered, the general path reproduces the hard-wired FRW_ENC_MONTGOMERY byte for byte in every call
     that takes a field encoding;
  3. a batch of more than one grid round in a foreign field against the same call's canonical output;
  4. the 160-bit extremes; 5. statuses; 6. the compact round trip; 7. refusals and the registry; 8. the example."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import field_cases as F
import frw_testlib as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = T.Q


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(torch.device("cuda:0"))


def _ints(t):
    """int64 device tensor [..., 4] -> Python integers, row-major"""
    return T.limbs_to_ints(t.cpu().numpy().view(np.uint64))


def _witness(engine, logn, sig, pk, hm, enc):
    """frw_witness_ntt_verify_dev -> (witness, instance, status) device tensors, synchronised"""
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    L = frw.layout(logn)
    sig, pk, hm = (np.ascontiguousarray(a, dtype=np.uint16).reshape(-1, L.n) for a in (sig, pk, hm))
    batch = sig.shape[0]
    wit = torch.full((batch, L.num_witness, 4), -1, dtype=torch.int64, device=dev)
    inst = torch.full((batch, L.num_instance, 4), -1, dtype=torch.int64, device=dev)
    st = torch.full((batch,), -7, dtype=torch.int32, device=dev)
    engine.witness_ntt_verify_dev(logn, batch, _dev(sig), _dev(pk), _dev(hm), wit, inst, st, enc, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return wit, inst, st


def _oracle_system(p, logn, sig, pk, hm):
    from oracle import falcon_gadgets as G
    from oracle.ark_sim import ConstraintSystem
    cs = ConstraintSystem(p)
    G.FalconNTTVerificationCircuit([int(x) for x in sig], [int(x) for x in pk], [int(x) for x in hm], logn).generate_constraints(cs)
    return cs


# ---- 1. oracle parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,logn,count", [("bn254", 9, 2), ("ed25519_l", 9, 2), ("pallas", 9, 2), ("bn254", 10, 1)])
def test_witness_equals_the_oracle_over_that_field(engine, name, logn, count):
    p = F.MODULI[name]
    enc = engine.field_encoding(p)
    rng = random.Random(1000 + logn)
    triples = [T.random_triple(logn, rng) for _ in range(count)]
    sig, pk, hm = (np.stack([t[k] for t in triples]) for k in range(3))
    wit, inst, st = _witness(engine, logn, sig, pk, hm, enc)
    assert st.tolist() == [0] * count
    for k in range(count):
        cs = _oracle_system(p, logn, sig[k], pk[k], hm[k])
        assert cs.is_satisfied()
        assert _ints(wit[k]) == [F.mont(v, p) for v in cs.witness_assignment], (name, k)
        assert _ints(inst[k]) == [F.mont(v, p) for v in cs.instance_assignment], (name, k)


# ---- 2. the general path reproduces the hard-wired one ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bls_enc(engine):
    import falcon_r1cs_amd as frw
    enc = engine.field_encoding(F.BLS12_381)
    assert frw.ENC_FIELD_BASE <= enc < frw.ENC_FIELD_BASE + frw.MAX_FIELDS
    return enc


@pytest.mark.parametrize("logn", [9, 10])
@pytest.mark.parametrize("batch", [1, 257])
def test_bls12_381_registered_witness_equals_montgomery(engine, bls_enc, logn, batch):
    """batch 1: the all-split launch; 257: more workgroups than one round and a ragged tail"""
    import torch
    import falcon_r1cs_amd as frw
    sig, pk, hm = frw.synth_triples(logn, batch, seed=381 + logn)
    want = _witness(engine, logn, sig, pk, hm, frw.ENC_MONTGOMERY)
    got = _witness(engine, logn, sig, pk, hm, bls_enc)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert not got[2].any()
    if batch == 1:                       # the host-buffer form takes the encoding too
        hw, hi, hs = engine.witness_ntt_verify(logn, sig, pk, hm, bls_enc, strict=True)
        assert np.array_equal(hw.view(np.int64), want[0].cpu().numpy()) and np.array_equal(hi.view(np.int64), want[1].cpu().numpy())
        assert engine.launch_shape(logn, 32768, bls_enc)["grid"] > 0


@pytest.mark.parametrize("logn", [9, 10])
def test_bls12_381_registered_ntt_modq_equals_montgomery(engine, bls_enc, logn):
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    n, batch = 1 << logn, 65
    poly, _, _ = frw.synth_triples(logn, batch, seed=65)
    outs = []
    for enc in (frw.ENC_MONTGOMERY, bls_enc):
        wit = torch.full((batch, 29 * n, 4), -1, dtype=torch.int64, device=dev)
        ntt = torch.full((batch, n), -1, dtype=torch.int16, device=dev)
        st = torch.full((batch,), -7, dtype=torch.int32, device=dev)
        engine.ntt_modq_dev(logn, batch, _dev(poly), wit, ntt, st, enc, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append((wit, ntt, st))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert not outs[1][2].any()
    hw, hn, hs = engine.ntt_modq(logn, poly[:3], bls_enc)                   # host-buffer form
    assert np.array_equal(hw.view(np.int64), outs[0][0][:3].cpu().numpy()) and not hs.any()


def _gadget_inputs():
    """the inputs of tests/test_gpu_parity.py::test_standalone_gadget_blocks_match_gadget_oracle"""
    import falcon_r1cs_amd as frw
    rng = random.Random(8)
    q = Q
    cases = {
        frw.G_LESS_THAN_Q: [42, 0, 1 << 12, 1 << 13, q - 1, q, q + 1, q * 10000] + [rng.randrange(1 << 15) for _ in range(150)],
        frw.G_MOD_Q: [6, 0, q, q + 1, (1 << 160) - 1, F.LADDER_MAX] + [rng.randrange(1 << 160) for _ in range(150)]
                     + [rng.randrange(1 << 30) for _ in range(50)],
        frw.G_L2_ELEM: [42, 0, 6143, 6144, 6145, q - 1, q] + [rng.randrange(q) for _ in range(150)],
        frw.G_NORM_BOUND_512: [42, 0, 1 << 25, 34034725, 34034726, 34034727, 1 << 26, 1 << 27] + [rng.randrange(1 << 27) for _ in range(150)],
        frw.G_NORM_BOUND_1024: [42, 0, 1 << 26, 70265241, 70265242, 70265243, 1 << 27] + [rng.randrange(1 << 27) for _ in range(150)],
    }
    pairs = [(6, 36), (0, 100), (100, 0), (5, q - 1)] + [(rng.randrange(1 << 30), rng.randrange(1 << 30)) for _ in range(150)] + [(q - 1, (q - 1) ** 2)]
    return cases, pairs


def test_bls12_381_registered_gadgets_equal_montgomery(engine, bls_enc):
    import falcon_r1cs_amd as frw
    cases, pairs = _gadget_inputs()
    assert len(cases) == 5
    for kind, vals in cases.items():
        want, wst = engine.gadget(kind, vals, encoding=frw.ENC_MONTGOMERY)
        got, gst = engine.gadget(kind, vals, encoding=bls_enc)
        assert np.array_equal(got, want) and np.array_equal(gst, wst), kind
    a, b = [x for x, _ in pairs], [y for _, y in pairs]
    want, wst = engine.gadget(frw.G_ADD_MOD, a, b, encoding=frw.ENC_MONTGOMERY)
    got, gst = engine.gadget(frw.G_ADD_MOD, a, b, encoding=bls_enc)
    assert np.array_equal(got, want) and np.array_equal(gst, wst)


@pytest.mark.parametrize("logn", [9, 10])
@pytest.mark.parametrize("circuit", [0, 1, 2])
def test_bls12_381_registered_statement_equals_montgomery(engine, bls_enc, circuit, logn):
    """circuits 0 and 1 take the NTT form, 2 the coefficient form; 37 statements = 74 work items"""
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    n, batch = 1 << logn, 37
    _, pk, hm = frw.synth_triples(logn, batch, seed=37 + circuit)
    pk = pk.copy()
    pk[5, n - 1] = Q                                  # one refused statement: zeros, under either encoding
    outs = []
    for enc in (frw.ENC_MONTGOMERY, bls_enc):
        inst = torch.full((batch, 2 * n + 1, 4), -1, dtype=torch.int64, device=dev)
        st = torch.full((batch,), -7, dtype=torch.int32, device=dev)
        engine.statement_dev(circuit, logn, batch, _dev(pk), _dev(hm), inst, st, enc, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append((inst, st))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert outs[1][1].tolist() == [0] * 5 + [frw.ST_COEFF_RANGE] + [0] * 31
    hi, hs = engine.statement(circuit, logn, pk[:4], hm[:4], bls_enc)         # host-buffer form
    assert np.array_equal(hi.view(np.int64), outs[0][0][:4].cpu().numpy())


def _signed_cases():
    with open(os.path.join(ROOT, "tests", "golden", "falcon_signed.json")) as f:
        return json.load(f)["cases"]


def test_bls12_381_registered_statement_from_bytes_equals_montgomery(engine, bls_enc):
    import torch
    import falcon_r1cs_amd as frw
    for logn in (9, 10):
        sel = [c for c in _signed_cases() if c["logn"] == logn]
        assert len(sel) == 2
        pkb = [bytes.fromhex(c["pk_bytes"]) for c in sel]
        non = [bytes.fromhex(c["sig_bytes"])[1:41] for c in sel]
        msgs = [bytes.fromhex(c["msg"]) for c in sel]
        want, wst = engine.statement_from_bytes_dev(0, logn, pkb, non, msgs, frw.ENC_MONTGOMERY)
        got, gst = engine.statement_from_bytes_dev(0, logn, pkb, non, msgs, bls_enc)
        torch.cuda.synchronize()
        assert torch.equal(got, want) and torch.equal(gst, wst) and not gst.any()
        hi, hs = engine.statement_from_bytes(0, logn, pkb, non, msgs, bls_enc)
        assert np.array_equal(hi.view(np.int64), want.cpu().numpy()) and not hs.any()


def _compact(engine, logn, sig, pk, hm):
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    batch = sig.shape[0]
    CL = frw.compact_layout(logn)
    comp = torch.full((batch, CL.bytes_per_signature), 0x5A, dtype=torch.uint8, device=dev)
    st = torch.full((batch,), -7, dtype=torch.int32, device=dev)
    engine.witness_ntt_verify_compact_dev(logn, batch, _dev(sig), _dev(pk), _dev(hm), comp, st, torch.cuda.current_stream().cuda_stream)
    return comp, st


@pytest.mark.parametrize("logn", [9, 10])
def test_expand_field_dev_with_bls12_381_equals_expand_dev(engine, bls_enc, logn):
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    L = frw.layout(logn)
    batch = 9
    sig, pk, hm = frw.synth_triples(logn, batch, seed=99)
    comp, st = _compact(engine, logn, sig, pk, hm)
    s0 = torch.cuda.current_stream().cuda_stream
    w = [torch.full((batch, L.num_witness, 4), -1, dtype=torch.int64, device=dev) for _ in range(2)]
    i = [torch.full((batch, L.num_instance, 4), -1, dtype=torch.int64, device=dev) for _ in range(2)]
    engine.expand_dev(logn, batch, comp, w[0], i[0], s0)
    engine.expand_field_dev(logn, batch, comp, bls_enc, w[1], i[1], s0)
    torch.cuda.synchronize()
    assert not st.any()
    assert torch.equal(w[0], w[1]) and torch.equal(i[0], i[1])


# ---- 3. a larger batch in a foreign field ----------------------------------------------------------------------------------------------
def test_bn254_batch_of_257_against_the_canonical_output(engine):
    import torch
    import falcon_r1cs_amd as frw
    p, logn, batch = F.BN254, 9, 257
    enc = engine.field_encoding(p)
    sig, pk, hm = frw.synth_triples(logn, batch, seed=254257)
    canon = _witness(engine, logn, sig, pk, hm, frw.ENC_CANONICAL)
    field = _witness(engine, logn, sig, pk, hm, enc)
    assert not canon[2].any() and torch.equal(canon[2], field[2])
    one = _dev(np.array(F.limbs4(F.consts(p)["one"]), dtype=np.uint64))
    unit = torch.tensor([1, 0, 0, 0], dtype=torch.int64, device=one.device)
    rng = random.Random(20000)
    for c, f in ((canon[0], field[0]), (canon[1], field[1])):
        c, f = c.view(-1, 4), f.view(-1, 4)
        is_zero = (c == 0).all(dim=1)
        is_one = (c == unit).all(dim=1)
        assert int(is_zero.sum()) > 0 and int(is_one.sum()) > 0
        assert not f[is_zero].any()                                             # every zero element: all zero
        assert bool((f[is_one] == one).all())                                   # every one element: `one`, limb-wise
        other = torch.nonzero(~(is_zero | is_one)).flatten()
        pick = other[torch.tensor(rng.sample(range(other.numel()), min(20000, other.numel())), device=other.device)]
        assert _ints(f[pick]) == [F.mont(v, p) for v in _ints(c[pick])]


# ---- 4. extremes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bn254", "2^255-19"])
def test_the_160_bit_extremes(engine, name):
    """the all-(q - 1) polynomial drives the un-reduced ladder of Falcon-1024 to its 160-bit maximum; FRW_G_MOD_Q takes 2^160 - 1"""
    import torch
    import falcon_r1cs_amd as frw
    from oracle import falcon_gadgets as G
    from oracle.ark_sim import ConstraintSystem, FpVar
    dev = torch.device("cuda:0")
    p = F.MODULI[name]
    enc = engine.field_encoding(p)
    logn, n = 10, 1024
    poly = np.full((1, n), Q - 1, dtype=np.uint16)
    wit = torch.full((1, 29 * n, 4), -1, dtype=torch.int64, device=dev)
    ntt = torch.full((1, n), -1, dtype=torch.int16, device=dev)
    st = torch.full((1,), -7, dtype=torch.int32, device=dev)
    engine.ntt_modq_dev(logn, 1, _dev(poly), wit, ntt, st, enc, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    cs = ConstraintSystem(p)
    vs = G.alloc_vars(cs, [Q - 1] * n, "Witness")
    w0 = cs.num_witness_variables()
    G.ntt_circuit(cs, vs, G.const_q_power_vars(cs, logn), G.ntt_param_var(cs, logn), logn)
    want = cs.witness_assignment[w0:]
    assert len(want) == 29 * n and max(want[0::29]).bit_length() >= 146 and cs.is_satisfied()
    assert st.tolist() == [0]
    assert _ints(wit[0]) == [F.mont(v, p) for v in want]
    assert ntt[0].tolist() == want[1::29]
    # mod_q on 2^160 - 1 and on the ladder maximum
    for a in ((1 << 160) - 1, F.LADDER_MAX):
        cs = ConstraintSystem(p)
        v = FpVar.new_witness(cs, a)
        w0 = cs.num_witness_variables()
        G.mod_q(cs, v, FpVar.constant(cs, Q))
        blocks, gst = engine.gadget(frw.G_MOD_Q, [a], encoding=enc)
        assert not gst.any()
        assert T.limbs_to_ints(blocks[0]) == [F.mont(x, p) for x in cs.witness_assignment[w0:]]
        assert T.limbs_to_ints(blocks[0])[0] == F.mont(a // Q, p)


# ---- 5. statuses -----------------------------------------------------------------------------------------------------------------------
def test_statuses_and_zero_fill_as_under_montgomery(engine):
    import falcon_r1cs_amd as frw
    p, logn = F.BN254, 9
    enc = engine.field_encoding(p)
    rng = random.Random(5)
    good = T.random_triple(logn, rng)
    loud = T.random_triple(logn, rng, scale=1.6)                             # norm above the bound: written, FRW_ST_NORM_BOUND
    bad_sig = good[0].copy()
    bad_sig[100] = Q                                                         # coefficient >= q: zero-filled, FRW_ST_COEFF_RANGE
    sig, pk, hm = np.stack([good[0], bad_sig, loud[0]]), np.stack([good[1], good[1], loud[1]]), np.stack([good[2], good[2], loud[2]])
    mw, mi, ms = _witness(engine, logn, sig, pk, hm, frw.ENC_MONTGOMERY)
    fw, fi, fs = _witness(engine, logn, sig, pk, hm, enc)
    assert fs.tolist() == ms.tolist() == [frw.ST_OK, frw.ST_COEFF_RANGE, frw.ST_NORM_BOUND]
    assert not fw[1].any() and not fi[1].any()
    rinv_bls, rinv_p = pow(1 << 256, -1, F.BLS12_381), pow(1 << 256, -1, p)
    for k in (0, 2):
        assert [v * rinv_p % p for v in _ints(fw[k])] == [v * rinv_bls % F.BLS12_381 for v in _ints(mw[k])], k
        assert [v * rinv_p % p for v in _ints(fi[k])] == [v * rinv_bls % F.BLS12_381 for v in _ints(mi[k])], k
    with pytest.raises(frw.FrwError) as ei:                                  # strict host-buffer form: FRW_E_RANGE, as under FRW_ENC_MONTGOMERY
        engine.witness_ntt_verify(logn, sig, pk, hm, enc, strict=True)
    assert ei.value.code == -5


# ---- 6. compact round trip -------------------------------------------------------------------------------------------------------------
def test_compact_then_expand_field_equals_the_direct_call(engine):
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    p, logn, batch = F.BN254, 9, 5
    enc = engine.field_encoding(p)
    L = frw.layout(logn)
    sig, pk, hm = frw.synth_triples(logn, batch, seed=55)
    sig = sig.copy()
    sig[3, 7] = 0xFFFF                                                       # one rejected signature
    dw, di, ds = _witness(engine, logn, sig, pk, hm, enc)
    comp, cst = _compact(engine, logn, sig, pk, hm)
    w = torch.full((batch, L.num_witness, 4), -1, dtype=torch.int64, device=dev)
    i = torch.full((batch, L.num_instance, 4), -1, dtype=torch.int64, device=dev)
    engine.expand_field_dev(logn, batch, comp, enc, w, i, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert ds.tolist() == cst.tolist() == [0, 0, 0, frw.ST_COEFF_RANGE, 0]
    assert torch.equal(w, dw) and torch.equal(i, di)
    assert not w[3].any() and not i[3].any()
    hw, hi = frw.expand_field_host(p, logn, comp.cpu().numpy())              # and the host expansion
    assert np.array_equal(hw.view(np.int64), dw.cpu().numpy()) and np.array_equal(hi.view(np.int64), di.cpu().numpy())


# ---- 7. refusals and the registry ------------------------------------------------------------------------------------------------------
def test_refusals_and_the_registry(engine):
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    logn = 9
    L = frw.layout(logn)
    a = frw.WitnessEngine(0)
    b = frw.WitnessEngine(0)
    try:
        enc = a.field_encoding(F.BN254)
        assert enc == frw.ENC_FIELD_BASE and a.field_encoding(F.BN254) == enc            # twice: the same id
        assert a.field_encoding(F.PALLAS) == enc + 1 and a.field_encoding(F.BN254) == enc
        sig, pk, hm = frw.synth_triples(logn, 1, seed=7)
        d = [_dev(x) for x in (sig, pk, hm)]
        inst = torch.zeros((1, L.num_instance, 4), dtype=torch.int64, device=dev)
        st = torch.full((1,), -7, dtype=torch.int32, device=dev)
        big = torch.zeros((1, frw.layout_schoolbook(logn).num_witness, 4), dtype=torch.int64, device=dev)

        def refused(fn, *args):
            with pytest.raises(frw.FrwError) as ei:
                fn(*args)
            assert ei.value.code == -1
        # the dual and schoolbook witness calls and the aggregate statement know BLS12-381 only
        refused(a.witness_dual_ntt_verify_dev, logn, 1, d[0], d[1], d[2], big, inst, st, enc, 0)
        refused(a.witness_schoolbook_verify_dev, logn, 1, d[0], d[1], d[2], big, inst, st, enc, 0)
        refused(a.witness_dual_ntt_verify, logn, sig, pk, hm, enc)
        refused(a.witness_schoolbook_verify, logn, sig, pk, hm, enc)
        agg = a.r1cs_load_aggregate([9, 9])
        ainst = torch.zeros((1 + 4 * 512, 4), dtype=torch.int64, device=dev)
        ast = torch.full((2,), -7, dtype=torch.int32, device=dev)
        two = [_dev(np.concatenate([x, x])) for x in (pk, hm)]
        refused(a.aggregate_statement_dev, agg, two[0], two[1], None, None, ainst, ast, enc, 0)
        a.aggregate_statement_dev(agg, two[0], two[1], None, None, ainst, ast, frw.ENC_MONTGOMERY, 0)      # (the call itself is sound)
        torch.cuda.synchronize()
        a.r1cs_free(agg)
        assert ast.tolist() == [0, 0]
        # an id nobody registered, and one registered on another context
        refused(a.witness_ntt_verify_dev, logn, 1, d[0], d[1], d[2], big, inst, st, enc + 2, 0)
        refused(b.witness_ntt_verify_dev, logn, 1, d[0], d[1], d[2], big, inst, st, enc, 0)
        refused(b.expand_field_dev, logn, 1, big, enc, big, inst, 0)
        refused(a.expand_field_dev, logn, 1, big, frw.ENC_MONTGOMERY, big, inst, 0)
        refused(b.launch_shape, logn, 1, enc)
        refused(a.ntt_modq_dev, logn, 1, d[0], big, d[1], st, enc + 2, 0)
        refused(a.statement_dev, 0, logn, 1, d[1], d[2], inst, st, frw.ENC_FIELD_BASE + frw.MAX_FIELDS, 0)
        assert st.tolist() == [-7] and not inst.any()                                    # nothing was launched
        # inadmissible moduli
        for p in F.REFUSED.values():
            refused(a.field_encoding, p)
        # eight distinct moduli fit, the ninth does not; the eight stay usable
        eight = list(F.MODULI.values()) + [(1 << 200) + 235]
        ids = [b.field_encoding(p) for p in eight]
        assert ids == list(range(frw.ENC_FIELD_BASE, frw.ENC_FIELD_BASE + 8))
        refused(b.field_encoding, (1 << 200) + 237)
        assert [b.field_encoding(p) for p in eight] == ids
        b.witness_ntt_verify_dev(logn, 1, d[0], d[1], d[2], big, inst, st, ids[7], 0)
        torch.cuda.synchronize()
        assert st.tolist() == [0] and _ints(inst[0, :1]) == [F.consts(eight[7])["one"]]
    finally:
        a.close()
        b.close()


# ---- 8. the example --------------------------------------------------------------------------------------------------------------------
def test_witness_bn254_example_exits_zero():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "witness_bn254.py"), os.path.join(ROOT, "tests", "golden", "falcon_signed.json")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "satisfied: True, bytes equal: True" in out.stdout
