"""The schoolbook circuit on the device: witness_schoolbook_verify_kernel bit for bit against the ORACLE
(oracle/falcon_gadgets.py::FalconSchoolBookVerificationCircuit on oracle/ark_sim.py, live at Falcon-512 and by the committed
digests of tests/golden/schoolbook_*.json at Falcon-1024), the host mirror's independently emitted constraint system
evaluated on the device over the kernel's witness, the witness map, and one Falcon-512 proof made and verified.

The proof is held to the product's own verifier and to the oracle's pairing-based verify_proof (as tests/test_examples.py does),
not to the prover restated in the exponent: setup_exponents over 312,882 variables and a 2^19 domain is minutes of Python."""
import random

import numpy as np
import pytest

import frw_testlib as T
import schoolbook_ref as S

pytestmark = pytest.mark.gpu
Q = S.Q
ENCODINGS = [(0, "canonical"), (1, "montgomery")]


def _dev_call(engine, logn, sig, pk, hm, enc, fill=-1):
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    L = frw.layout_schoolbook(logn)
    sig, pk, hm = (np.ascontiguousarray(a, dtype=np.uint16).reshape(-1, L.n) for a in (sig, pk, hm))
    batch = sig.shape[0]
    d = [torch.from_numpy(a.view(np.int16)).to(dev) for a in (sig, pk, hm)]
    wit = torch.full((batch, L.num_witness, 4), fill, dtype=torch.int64, device=dev)
    inst = torch.full((batch, L.num_instance, 4), fill, dtype=torch.int64, device=dev)
    st = torch.full((batch,), -1, dtype=torch.int32, device=dev)
    engine.witness_schoolbook_verify_dev(logn, batch, d[0], d[1], d[2], wit, inst, st, enc, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return wit, inst, st


def _first_difference(got, want):
    a, b = np.frombuffer(got, dtype=np.uint64).reshape(-1, 4), np.frombuffer(want, dtype=np.uint64).reshape(-1, 4)
    bad = np.nonzero((a != b).any(axis=1))[0]
    return "first differing element %d of %d differing; got %s want %s" % (bad[0], len(bad), a[bad[0]], b[bad[0]]) if len(bad) else "equal"


@pytest.mark.parametrize("enc,name", ENCODINGS)
def test_falcon512_witness_equals_the_live_oracle(engine, enc, name):
    cs = S.fixture_cs(9)
    sig, pk, hm = S.triple(9, S.SEEDS[9][0])
    want_w, want_i = S.encoded(cs, bool(enc))
    wit, inst, st = engine.witness_schoolbook_verify(9, sig[None], pk[None], hm[None], enc, strict=True)
    assert st.tolist() == [0]
    assert inst.tobytes() == want_i, _first_difference(inst.tobytes(), want_i)
    assert wit.tobytes() == want_w, _first_difference(wit.tobytes(), want_w)


@pytest.mark.parametrize("enc,name", ENCODINGS)
@pytest.mark.parametrize("logn,batch,odd_slot", [(9, 1, None), (10, 1, None), (9, 3, 1), (9, 37, 20), (10, 2, 1)])
def test_witness_equals_the_golden_digests(engine, logn, batch, odd_slot, enc, name):
    """Ragged batches: the first fixture triple repeated, slot `odd_slot` replaced by the second one; every slot is hashed."""
    g = S.golden(logn)
    triples = [S.golden_triple(g, 0), S.golden_triple(g, 1)]
    which = [1 if k == odd_slot else 0 for k in range(batch)]
    sig, pk, hm = (np.stack([triples[w][j] for w in which]) for j in range(3))
    wit, inst, st = _dev_call(engine, logn, sig, pk, hm, enc)
    assert st.tolist() == [0] * batch
    wit_h, inst_h = wit.cpu().numpy(), inst.cpu().numpy()
    for k, w in enumerate(which):
        want = g["triples"][w]["sha256"][name]
        assert S.sha(inst_h[k].tobytes()) == want["instance"], (k, w)
        assert S.sha(wit_h[k].tobytes()) == want["witness"], (k, w)
    if batch <= 3:          # the host-buffer form agrees byte for byte
        hw, hi, hs = engine.witness_schoolbook_verify(logn, sig, pk, hm, enc, strict=True)
        assert hs.tolist() == [0] * batch and hw.tobytes() == wit_h.tobytes() and hi.tobytes() == inst_h.tobytes()


def _edge(case):
    n = 512
    rng = random.Random(77)
    sig, pk, hm = S.triple(9, S.SEEDS[9][1])
    if case == "pk zero":
        pk = np.zeros(n, dtype=np.uint16)
    elif case == "sig zero":
        sig = np.zeros(n, dtype=np.uint16)
    elif case == "hm zero":
        hm = np.zeros(n, dtype=np.uint16)
        sig = np.array([rng.randrange(Q) for _ in range(n)], dtype=np.uint16)
    elif case == "sig and pk all q - 1":
        sig = np.full(n, Q - 1, dtype=np.uint16)
        pk = np.full(n, Q - 1, dtype=np.uint16)
    return sig, pk, hm


@pytest.mark.parametrize("case", ["pk zero", "sig zero", "hm zero", "sig and pk all q - 1"])
def test_edge_polynomials_equal_the_live_oracle(engine, case):
    import falcon_r1cs_amd as frw
    sig, pk, hm = _edge(case)
    cs = S.oracle_cs(sig, pk, hm, 9, strict=False)
    n = 512
    if case == "sig zero":
        assert S.tail_counts(cs, 9) == (0, n)                    # c = 0: every column takes the hm >= c tail
    if case == "pk zero":                                        # b = q (not reduced) or 0 in every product
        assert set(cs.witness_assignment[29 * n + 2:29 * n + 2 + n]) <= {0} | {int(s) * Q for s in sig}
    norm = T.centred_norm(sig, [v for v in cs.witness_assignment[n:29 * n:28]])
    want_st = frw.ST_NORM_BOUND if norm >= T.SIG_L2_BOUND[9] else frw.ST_OK
    if case == "sig and pk all q - 1":
        assert want_st == frw.ST_NORM_BOUND
    for enc, name in ENCODINGS:
        want_w, want_i = S.encoded(cs, bool(enc))
        wit, inst, st = engine.witness_schoolbook_verify(9, sig[None], pk[None], hm[None], enc, strict=False)
        assert st.tolist() == [want_st]
        assert inst.tobytes() == want_i, _first_difference(inst.tobytes(), want_i)
        assert wit.tobytes() == want_w, _first_difference(wit.tobytes(), want_w)
    if want_st == frw.ST_NORM_BOUND:                             # strict mode: the host-buffer form refuses
        with pytest.raises(frw.FrwError) as e:
            engine.witness_schoolbook_verify(9, sig[None], pk[None], hm[None], 1, strict=True)
        assert e.value.code == frw.engine.E_RANGE


@pytest.mark.parametrize("which", ["sig", "pk", "hm"])
def test_a_coefficient_equal_to_q_zero_fills_that_slot_only(engine, which):
    import falcon_r1cs_amd as frw
    g = S.golden(9)
    base = S.golden_triple(g, 0)
    arrs = [np.stack([a, a, a]) for a in base]
    arrs[("sig", "pk", "hm").index(which)][1, 300] = Q
    wit, inst, st = _dev_call(engine, 9, *arrs, 1)
    assert st.tolist() == [0, frw.ST_COEFF_RANGE, 0]
    wit_h, inst_h = wit.cpu().numpy(), inst.cpu().numpy()
    assert not wit_h[1].any() and not inst_h[1].any()
    want = g["triples"][0]["sha256"]["montgomery"]
    for k in (0, 2):
        assert S.sha(wit_h[k].tobytes()) == want["witness"] and S.sha(inst_h[k].tobytes()) == want["instance"]


def test_compact_encoding_and_bad_arguments_are_refused(engine):
    import ctypes as C
    import falcon_r1cs_amd as frw
    lib = frw.load_library()
    p = C.c_void_p(16)
    ctx = engine._ctx
    assert lib.frw_witness_schoolbook_verify_dev(ctx, 9, 1, p, p, p, frw.ENC_COMPACT, p, p, p, None) == -1
    assert lib.frw_witness_schoolbook_verify(ctx, 9, 1, p, p, p, frw.ENC_COMPACT, p, p, p, 0) == -1
    assert lib.frw_witness_schoolbook_verify_dev(ctx, 8, 1, p, p, p, 1, p, p, p, None) == -1
    assert lib.frw_witness_schoolbook_verify_dev(ctx, 9, 1, None, p, p, 1, p, p, p, None) == -1
    assert lib.frw_witness_schoolbook_verify_dev(ctx, 9, 0, None, None, None, 1, None, None, None, None) == 0     # empty batch


def _mont(v):
    return T.ints_to_limbs([v * S.G.R_MONT % S.P])[0].view(np.int64)


def _value(t):
    return T.limbs_to_ints(t.cpu().numpy().view(np.uint64).reshape(1, 4))[0] * pow(S.G.R_MONT, -1, S.P) % S.P


@pytest.mark.parametrize("walk", ["flattened rows", "CSR walk"])
@pytest.mark.parametrize("logn,batch", [(9, 64), (10, 8)])
def test_device_witness_satisfies_the_mirror_s_system_on_the_device(engine, monkeypatch, logn, batch, walk):
    """frw_r1cs_load(FRW_CIRCUIT_SCHOOLBOOK): the matrices come from the host mirror's generate_constraints in setup mode,
    independently of the kernel's closed form.  Every signature of a synthetic batch satisfies them; five planted faults are
    each flagged in exactly their own signature."""
    if walk == "CSR walk":
        monkeypatch.setenv("FRW_R1CS_NO_FLAT", "1")
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    L = frw.layout_schoolbook(logn)
    n = L.n
    sig, pk, hm = frw.synth_triples(logn, batch, seed=8080 + logn)
    wit, inst, st = _dev_call(engine, logn, sig, pk, hm, 1)
    assert st.tolist() == [0] * batch
    r = engine.r1cs_load(S.CIRCUIT_SCHOOLBOOK, logn)
    try:
        info = engine.r1cs_info(r)
        assert (int(info.num_instance), int(info.num_witness), int(info.num_constraints)) == S.counts(logn)
        assert int(info.log_domain_size) == (19 if logn == 9 else 21)
        bad = torch.full((batch,), -1, dtype=torch.int32, device=dev)
        engine.r1cs_check_dev(r, batch, wit, inst, bad, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bad.tolist() == [0] * batch
        col = 29 * n + 5 * (n + 34)                                  # column 5
        one = torch.from_numpy(_mont(1)).to(dev)
        zero = torch.zeros(4, dtype=torch.int64, device=dev)
        # signature 1: a boolean of ltq(v[9]) flipped
        b = wit[1, n + 9 * 28 + 3]
        wit[1, n + 9 * 28 + 3] = zero if bool((b != 0).any()) else one
        # signature 2: product 17 of column 5, + 1;  signature 3: t of column 5, + 1
        wit[2, col + 2 + 17] = torch.from_numpy(_mont(_value(wit[2, col + 2 + 17]) + 1)).to(dev)
        wit[3, col] = torch.from_numpy(_mont(_value(wit[3, col]) + 1)).to(dev)
        # signature 4: the two multipliers of column 5 swapped;  signature 5: the public hm[5] changed
        m1, m2 = wit[4, col + n + 30].clone(), wit[4, col + n + 32].clone()
        wit[4, col + n + 30], wit[4, col + n + 32] = m2, m1
        inst[5, 1 + n + 5] = torch.from_numpy(_mont((_value(inst[5, 1 + n + 5]) + 1) % Q)).to(dev)
        engine.r1cs_check_dev(r, batch, wit, inst, bad, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = bad.tolist()
        assert all(x > 0 for x in got[1:6]) and got[0] == 0 and got[6:] == [0] * (batch - 6), got
    finally:
        engine.r1cs_free(r)


def test_witness_map_and_one_proof(engine):
    """Falcon-512, two signatures: the witness map (2^19 domain) has no violated row, a zero top coefficient and equals the
    six-transform quotient; a key from frw_groth16_setup with fixed toxic values, proofs from frw_groth16_prove_dev, accepted
    by the product's verifier and by the oracle's pairing-based verify_proof, rejected with one public input changed."""
    import torch
    import falcon_r1cs_amd as frw
    from oracle import bls12_381 as E
    dev = torch.device("cuda:0")
    logn, batch = 9, 2
    g = S.golden(logn)
    sig, pk, hm = (np.stack([S.golden_triple(g, w)[j] for w in (0, 1)]) for j in range(3))
    wit, inst, st = _dev_call(engine, logn, sig, pk, hm, 1)
    assert st.tolist() == [0, 0]
    s0 = torch.cuda.current_stream().cuda_stream
    r = engine.r1cs_load(S.CIRCUIT_SCHOOLBOOK, logn)
    handle = None
    try:
        q = engine.qap_info(r)
        n = int(q.domain_size)
        assert n == 1 << 19
        per = int(q.workspace_bytes_per_signature)
        ws = torch.empty(batch * per, dtype=torch.uint8, device=dev)
        h = torch.full((batch, n, 4), -1, dtype=torch.int64, device=dev)
        hq = torch.full((batch, n, 4), -1, dtype=torch.int64, device=dev)
        bad = torch.full((batch,), -1, dtype=torch.int32, device=dev)
        badq = torch.full((batch,), -1, dtype=torch.int32, device=dev)
        engine.qap_witness_map_dev(r, batch, wit, inst, h, ws, ws.numel(), bad, s0)
        engine.qap_quotient_dev(r, batch, wit, inst, hq, ws, ws.numel(), badq, s0)
        torch.cuda.synchronize()
        assert bad.tolist() == [0, 0] and badq.tolist() == [0, 0]
        assert int(h[:, -1].abs().sum()) == 0
        assert torch.equal(h, hq)
        del h, hq, ws
        rng = random.Random(2026)
        toxic = [rng.randrange(2, E.R) for _ in range(5)]
        handle, vk = engine.groth16_setup(S.CIRCUIT_SCHOOLBOOK, logn, *toxic)
        rs = np.array([T.ints_to_limbs([rng.randrange(E.R), rng.randrange(E.R)]) for _ in range(batch)])
        ws_bytes = engine.groth16_workspace_bytes(handle, r, batch)
        pws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        proofs = torch.full((batch, 48), -1, dtype=torch.int64, device=dev)
        engine.groth16_prove_dev(handle, r, batch, wit, inst, rs, proofs, pws, ws_bytes, bad, s0)
        torch.cuda.synchronize()
        assert bad.tolist() == [0, 0]
        got = proofs.cpu().numpy().view(np.uint64)
        inst_h = inst.cpu().numpy().view(np.uint64)
        ver = frw.Groth16Verifier(vk)
        assert ver.verify(inst_h, got).tolist() == [1, 1]
        tampered = inst_h.copy()
        tampered[1, 1 + 512 + 8, 0] ^= np.uint64(2)                    # hm[8] of statement 1
        assert ver.verify(tampered, got).tolist() == [1, 0]
        ver.close()
        vk_pts = {"alpha_g1": E.from_limbs(vk["alpha_g1"]), "beta_g2": E.g2_from_limbs(vk["beta_g2"]),
                  "gamma_g2": E.g2_from_limbs(vk["gamma_g2"]), "delta_g2": E.g2_from_limbs(vk["delta_g2"]),
                  "gamma_abc_g1": [E.from_limbs(row) for row in vk["gamma_abc_g1"]]}
        r_inv = pow(S.G.R_MONT, -1, E.R)
        z0 = [v * r_inv % E.R for v in T.limbs_to_ints(inst_h[0])]
        proof0 = (E.from_limbs(got[0, :12]), E.g2_from_limbs(got[0, 12:36]), E.from_limbs(got[0, 36:]))
        assert E.verify_proof(vk_pts, z0[1:], proof0), "verify_proof rejects the device's proof"
        wrong = list(z0[1:])
        wrong[7] = (wrong[7] + 1) % E.R
        assert not E.verify_proof(vk_pts, wrong, proof0)
    finally:
        engine.r1cs_free(r)
        if handle is not None:
            engine.groth16_pk_free(handle)


def test_the_dev_call_is_capture_safe(engine):
    """One kernel, captured into a HIP graph and replayed on a second input set: digests equal the direct calls'."""
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    logn, batch = 9, 3
    L = frw.layout_schoolbook(logn)
    first, second = frw.synth_triples(logn, batch, seed=41), frw.synth_triples(logn, batch, seed=42)
    want = []
    for trip in (first, second):
        wit, inst, st = _dev_call(engine, logn, *trip, 1)
        dig = torch.zeros(batch, dtype=torch.int64, device=dev)
        engine.digest_dev(wit, L.num_witness * 4, batch, dig, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        want.append((dig.tolist(), inst.clone()))
    assert want[0][0] != want[1][0]
    d = [torch.from_numpy(a.view(np.int16)).to(dev) for a in first]
    wit = torch.zeros((batch, L.num_witness, 4), dtype=torch.int64, device=dev)
    inst = torch.zeros((batch, L.num_instance, 4), dtype=torch.int64, device=dev)
    st = torch.full((batch,), -1, dtype=torch.int32, device=dev)
    dig = torch.zeros(batch, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    allocs = engine.host_allocations()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        engine.witness_schoolbook_verify_dev(logn, batch, d[0], d[1], d[2], wit, inst, st, 1, side.cuda_stream)
    for k, trip in enumerate((first, second)):
        for t, a in zip(d, trip):
            t.copy_(torch.from_numpy(a.view(np.int16)))
        graph.replay()
        torch.cuda.synchronize()
        engine.digest_dev(wit, L.num_witness * 4, batch, dig, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert st.tolist() == [0] * batch
        assert dig.tolist() == want[k][0] and torch.equal(inst, want[k][1])
    assert engine.host_allocations() == allocs          # the _dev form allocates nothing
