"""Groth16 for constraint systems that come in as matrices (frw_r1cs_load_csr / frw_r1cs_load_file), on QAP domains from 2^1 up, against the
oracle: oracle/qap.py (matvec, witness_map) and oracle/bls12_381.py (setup_exponents, prove_exponents, verify_exponents), used as
tests/test_gpu_groth16.py uses them.

The systems are made by a seeded generator of SATISFIED systems: row i takes sparse A_i, B_i over variables that exist already, and
C_i is a fresh witness variable times a random coefficient (plus, where a test asks, terms over existing variables), its value solved
from <A_i, z> <B_i, z>.  Coefficients and free values are a mix of small ones and full-size ones (>= 2^250).  A system's coefficients come
from a pool: a dozen distinct ones keeps the flattened short-row kernel in play, four hundred send the system through the CSR walk.

What a check's bound is: none -- field arithmetic is exact, every comparison is word for word or byte for byte."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import frw_testlib as T
from oracle import bls12_381 as E
from oracle import qap

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = E.R
FR_R = (1 << 256) % P
R_INV = pow(FR_R, -1, P)


def _value(rng):
    """small or full-size, half and half"""
    return rng.randrange(1, 1 << 14) if rng.random() < 0.5 else rng.randrange(1 << 250, P)


class System:
    """A satisfied R1CS with its assignment.  mats: (A, B, C) as lists of rows [(coeff, column)]; z: the full assignment."""

    def __init__(self, num_constraints, num_instance, seed, num_free=4, pool=12, special=None, unused=0, small_free=0):
        rng = random.Random(seed)
        self.ni, self.nc = num_instance, num_constraints
        coeffs = [1, P - 1, 2] + [_value(rng) for _ in range(pool - 3)]
        # the public inputs and the free witness values, then (as the rows come) one solved value per row; `unused` more at the end
        z = [1] + [_value(rng) for _ in range(num_instance - 1)] + [rng.randrange(1, 1 << 28) for _ in range(small_free)] + \
            [_value(rng) for _ in range(num_free)]
        self.small_cols = list(range(num_instance, num_instance + small_free))
        a, b, c = [], [], []
        for row in range(num_constraints):
            existing = len(z)
            terms = lambda k: [(rng.choice(coeffs), rng.randrange(existing)) for _ in range(k)]
            ra, rb, rc = terms(rng.randrange(1, 4)), terms(rng.randrange(1, 3)), []
            if special and row in special:
                ra, rb, rc = special[row](rng, z, ra, rb, self)
            new_coeff = rng.choice(coeffs)
            want = qap.evaluate_constraint(ra, z) * qap.evaluate_constraint(rb, z) - qap.evaluate_constraint(rc, z)
            z.append(want * pow(new_coeff, -1, P) % P)
            a.append(ra)
            b.append(rb)
            c.append(rc + [(new_coeff, existing)])
        z += [_value(rng) for _ in range(unused)]
        self.mats, self.z = (a, b, c), z
        self.nw = len(z) - num_instance
        self.domain = qap.Domain(num_constraints + num_instance)

    def csr(self):
        out = []
        for m in self.mats:
            ptr = np.cumsum([0] + [len(r) for r in m]).astype(np.uint64)
            col = np.array([col for r in m for _, col in r], dtype=np.uint32)
            val = T.ints_to_limbs([coeff for r in m for coeff, _ in r]) if len(col) else np.zeros((0, 4), dtype=np.uint64)
            out.append((ptr, col, val))
        return out

    def load(self, engine):
        return engine.r1cs_load_csr(self.ni, self.nw, self.csr())


def _mont(values):
    return T.ints_to_limbs([v * FR_R % P for v in values])


def _dev(arr, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).copy()).to(dev)


def _canon(t):
    return [v * R_INV % P for v in T.limbs_to_ints(t.cpu().numpy().view(np.uint64))]


def _assignments(zs, ni, dev):
    """full assignments -> (witness [batch, W, 4], instance [batch, I, 4]) device tensors in ark-ff's bytes"""
    wit = np.stack([_mont(z[ni:]) for z in zs])
    inst = np.stack([_mont(z[:ni]) for z in zs])
    return _dev(wit, dev), _dev(inst, dev)


def _witness_map(engine, handle, wit, inst, in_flight=None, quotient=False):
    import torch
    q = engine.qap_info(handle)
    batch = wit.shape[0]
    per = int(q.workspace_bytes_per_signature)
    ws = torch.empty((in_flight or batch) * per, dtype=torch.uint8, device=wit.device)
    h = torch.full((batch, int(q.domain_size), 4), -1, dtype=torch.int64, device=wit.device)
    bad = torch.full((batch,), -1, dtype=torch.int32, device=wit.device)
    (engine.qap_quotient_dev if quotient else engine.qap_witness_map_dev)(handle, batch, wit, inst, h, ws, ws.numel(), bad,
                                                                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return h, bad


def _prove(engine, key, handle, wit, inst, rs):
    import torch
    batch = wit.shape[0]
    ws_bytes = engine.groth16_workspace_bytes(key, handle, batch)
    assert ws_bytes
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=wit.device)
    proofs = torch.full((batch, 48), -1, dtype=torch.int64, device=wit.device)
    bad = torch.full((batch,), -1, dtype=torch.int32, device=wit.device)
    engine.groth16_prove_dev(key, handle, batch, wit, inst, np.array([T.ints_to_limbs(x) for x in rs]), proofs, ws, ws_bytes, bad,
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return proofs, bad


def _expected_proof(oracle, pk, z, h, r, s):
    a, b, c, _ = E.prove_exponents(pk, z, h, r, s)
    assert E.verify_exponents(pk, z[1:len(pk["gamma_abc"])], (a, b, c)), "the restated prover's own proof does not verify"
    gen = oracle.g1_generator()
    return oracle.g1_scalar_mul(gen, a).tolist() + E.g2_to_limbs(E.g2_mul(E.G2, b)) + oracle.g1_scalar_mul(gen, c).tolist()


def _toxic(rng):
    return {k: rng.randrange(2, P) for k in ("alpha", "beta", "gamma", "delta", "t")}


def _setup(engine, handle, toxic, **kw):
    return engine.groth16_setup_r1cs(handle, toxic["alpha"], toxic["beta"], toxic["gamma"], toxic["delta"], toxic["t"], **kw)


# ---- 1. the export, loaded back, is the built-in handle -------------------------------------------------------------------------------
def test_the_export_loaded_back_is_the_built_in_handle(engine, tmp_path):
    import torch
    import falcon_r1cs_amd as frw
    from falcon_r1cs_amd import engine as eng_mod
    from test_r1cs_export import export
    dev = torch.device("cuda:0")
    logn, batch = 9, 3
    L = frw.layout(logn)
    export(0, logn, tmp_path / "ntt9.r1cs")
    loaded = engine.r1cs_load_file(tmp_path / "ntt9.r1cs")
    built_in = engine.r1cs_load(0, logn)
    keys = []
    try:
        i_l, i_b = engine.r1cs_info(loaded), engine.r1cs_info(built_in)
        for f in ("num_statements", "num_instance", "num_witness", "num_constraints", "log_domain_size", "witness_map_on_device"):
            assert getattr(i_l, f) == getattr(i_b, f), f
        assert (i_b.count_logn9, i_b.count_logn10) == (1, 0) and (i_l.count_logn9, i_l.count_logn10) == (0, 0)
        sig, pk_, hm = frw.synth_triples(logn, batch, seed=4711)
        dd = [torch.from_numpy(a.view(np.int16)).to(dev) for a in (sig, pk_, hm)]
        wit = torch.empty((batch, L.num_witness, 4), dtype=torch.int64, device=dev)
        inst = torch.empty((batch, L.num_instance, 4), dtype=torch.int64, device=dev)
        st = torch.empty(batch, dtype=torch.int32, device=dev)
        s0 = torch.cuda.current_stream().cuda_stream
        engine.witness_ntt_verify_dev(logn, batch, dd[0], dd[1], dd[2], wit, inst, st, 1, s0)
        got = []
        for handle in (loaded, built_in):
            abc = torch.full((batch, 3, L.num_constraints, 4), -1, dtype=torch.int64, device=dev)
            bad = torch.full((batch,), -1, dtype=torch.int32, device=dev)
            engine.r1cs_eval_dev(handle, batch, wit, inst, bad, abc, s0)
            h, bad_h = _witness_map(engine, handle, wit, inst)
            assert bad.tolist() == [0] * batch and bad_h.tolist() == [0] * batch
            got.append((abc, h))
        assert torch.equal(got[0][0], got[1][0]), "A z, B z, C z differ"
        assert torch.equal(got[0][1], got[1][1]), "h differs"
        rng = random.Random(1)
        toxic = _toxic(rng)
        rs = [[rng.randrange(P), rng.randrange(P)] for _ in range(batch)]
        proofs = []
        for handle in (loaded, built_in):
            key, _ = _setup(engine, handle, toxic, want_vk=False)
            keys.append(key)
            p, bad = _prove(engine, key, handle, wit, inst, rs)
            assert bad.tolist() == [0] * batch
            proofs.append(p)
        assert torch.equal(proofs[0], proofs[1]), "the proofs differ"
        # the calls that start from Falcon signatures know frw_r1cs_load's handles only: the loaded one has the counts and is refused
        assert engine.pok_prove_workspace_bytes(keys[1], built_in, 0, logn, 1, 1) > 0
        assert engine.pok_prove_workspace_bytes(keys[0], loaded, 0, logn, 1, 1) == 0
        d_pkb = torch.zeros(eng_mod.PK_LEN[logn], dtype=torch.uint8, device=dev)
        d_sgb = torch.zeros(eng_mod.SIG_LEN[logn], dtype=torch.uint8, device=dev)
        msgs = (torch.zeros(1, dtype=torch.uint8, device=dev), torch.tensor([0, 1], dtype=torch.int64, device=dev))
        with pytest.raises(frw.FrwError) as ei:
            engine.pok_prove_from_bytes_dev(keys[0], loaded, 0, logn, d_pkb, d_sgb, msgs, np.zeros((1, 2, 4), dtype=np.uint64), stream=s0)
        assert ei.value.code == -1
    finally:
        for k in keys:
            engine.groth16_pk_free(k)
        engine.r1cs_free(loaded)
        engine.r1cs_free(built_in)


# ---- 2. domain edges against the oracle ------------------------------------------------------------------------------------------------
# C + I; the number of instance variables (the constant one among them); whether the proof is held to the exponent prover's bytes
EDGES = [(2, 1, True), (3, 2, True), (4, 2, True), (8, 3, True), (64, 5, True), (4096, 5, False), (4097, 5, False), (8192, 5, False),
         (8193, 5, True)]


@pytest.mark.parametrize("total,ni,exact", EDGES, ids=["C+I=%d" % e[0] for e in EDGES])
def test_domain_edges_against_the_oracle(engine, oracle, total, ni, exact):
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    s = System(total - ni, ni, seed=1000 + total)
    n = s.domain.size
    assert n == 1 << max(1, (total - 1).bit_length())
    handle = s.load(engine)
    key = None
    try:
        info, q = engine.r1cs_info(handle), engine.qap_info(handle)
        assert (info.num_statements, info.count_logn9, info.count_logn10) == (1, 0, 0)
        assert (info.num_instance, info.num_witness, info.num_constraints) == (ni, s.nw, total - ni)
        assert info.log_domain_size == s.domain.log_size and info.witness_map_on_device == 1
        assert (q.log_domain_size, q.domain_size) == (s.domain.log_size, n)
        assert q.workspace_bytes_per_signature == 3 * (total - ni) * 32 + 3 * 32 * n + 64
        wit, inst = _assignments([s.z], ni, dev)
        h, bad = _witness_map(engine, handle, wit, inst)
        want_h = qap.witness_map(s.mats, ni, s.z)
        assert bad.tolist() == [0]
        assert _canon(h[0]) == want_h, "h differs from witness_map"
        if n < 1 << 14:                                             # one map on the small domains: the quotient call returns it too
            hq, badq = _witness_map(engine, handle, wit, inst, quotient=True)
            assert torch.equal(hq, h) and badq.tolist() == [0]
        rng = random.Random(2000 + total)
        toxic = _toxic(rng)
        key, vk = _setup(engine, handle, toxic)
        r, sb = rng.randrange(P), rng.randrange(P)
        proofs, badp = _prove(engine, key, handle, wit, inst, [[r, sb]])
        assert badp.tolist() == [0]
        got = proofs.cpu().numpy().view(np.uint64)
        if exact:
            pk = E.setup_exponents(s.mats, ni, s.nw, s.domain, toxic)
            assert got[0].tolist() == _expected_proof(oracle, pk, s.z, want_h, r, sb), "the proof differs from the exponent prover's points"
        ver = frw.Groth16Verifier(vk)
        inst_h = inst.cpu().numpy().view(np.uint64)
        assert ver.verify(inst_h, got).tolist() == [1]
        if ni > 1:
            tampered = inst_h.copy()
            tampered[0, ni - 1] = _mont([(s.z[ni - 1] + 1) % P])[0]
            assert ver.verify(tampered, got).tolist() == [0]
        ver.close()
    finally:
        if key is not None:
            engine.groth16_pk_free(key)
        engine.r1cs_free(handle)


# ---- 3. a batch on a small domain, in chunks, one statement violated ------------------------------------------------------------------------
def test_a_batch_on_a_small_domain_with_one_violated_statement(engine):
    import torch
    dev = torch.device("cuda:0")
    ni, total, batch = 5, 1000, 5
    # ONE system; five assignments: the same rows solved for other free values.  Its dozen coefficients keep it on the flattened short-row
    # kernel, which so meets an empty B row, an empty A row, a repeated column and a zero coefficient too
    special = {20: lambda rng, z, ra, rb, s: (ra, [], []), 21: lambda rng, z, ra, rb, s: ([], rb, []),
               22: lambda rng, z, ra, rb, s: ([(2, 3), (P - 1, 6), (0, 1), (2, 3)], rb, [])}
    systems = [System(total - ni, ni, seed=31, special=special)]
    rng = random.Random(32)
    zs = []
    for k in range(batch):
        z = [1] + [_value(rng) for _ in range(ni - 1 + 4)]
        for row in range(total - ni):
            (ca, cb, cc) = (systems[0].mats[m][row] for m in range(3))
            coeff, col = cc[-1]
            assert col == len(z)
            z.append(qap.evaluate_constraint(ca, z) * qap.evaluate_constraint(cb, z) * pow(coeff, -1, P) % P)
        zs.append(z)
    s = systems[0]
    assert s.domain.size == 1 << 10
    # statement 3: one witness element that later rows read is off by one
    victim = ni + 4 + 10
    zs[3][victim] = (zs[3][victim] + 1) % P
    az, bz, cz = qap.matvec(s.mats, zs[3])
    violated = sum(1 for x, y, w in zip(az, bz, cz) if x * y % P != w)
    assert violated >= 1
    handle = s.load(engine)
    try:
        wit, inst = _assignments(zs, ni, dev)
        h, bad = _witness_map(engine, handle, wit, inst, in_flight=2)                  # 2 + 2 + 1
        assert bad.tolist() == [0, 0, 0, violated, 0]
        for k in range(batch):
            assert _canon(h[k]) == qap.witness_map(s.mats, ni, zs[k]), "statement %d" % k
        # the same in one chunk: the same bytes
        h1, bad1 = _witness_map(engine, handle, wit, inst)
        assert torch.equal(h1, h) and torch.equal(bad1, bad)
        # ... and from host buffers (frw_qap_witness_map)
        hh, badh = engine.qap_witness_map(handle, wit.cpu().numpy().view(np.uint64), inst.cpu().numpy().view(np.uint64))
        assert np.array_equal(hh, h.cpu().numpy().view(np.uint64)) and badh.tolist() == bad.tolist()
    finally:
        engine.r1cs_free(handle)


# ---- 4. rows the Falcon circuits never show ----------------------------------------------------------------------------------------------
def test_rows_the_falcon_circuits_never_show(engine, oracle):
    import torch
    import falcon_r1cs_amd as frw
    from falcon_r1cs_amd import engine as eng_mod
    dev = torch.device("cuda:0")
    ni, nc = 5, 8995                                                # C + I = 9000: the 2^14 domain, the existing passes

    def full(rng):
        return rng.randrange(1 << 250, P)

    def long_a(rng, z, ra, rb, s):
        # 300 terms in A: variables whose values are full-size (solved values of earlier rows), coefficients full-size
        cols = [c for c in range(s.ni + 254, len(z)) if z[c] >> 250][:300]
        assert len(cols) == 300
        return [(full(rng), c) for c in cols], rb, []

    def long_c(rng, z, ra, rb, s):
        # 200 terms in C: 199 variables below 2^28, and the row's own fresh one (a solved, full-size value)
        cols = [rng.choice(s.small_cols) for _ in range(199)]
        assert all(z[c] < 1 << 28 for c in cols)
        return ra, rb, [(full(rng), c) for c in cols]

    special = {
        700: long_a,
        701: long_c,
        702: lambda rng, z, ra, rb, s: ([(3, 7), (full(rng), 9), (5, 7)], rb, []),            # a repeated column
        703: lambda rng, z, ra, rb, s: ([(0, 8), (full(rng), 11)], rb, []),                    # a zero coefficient
        704: lambda rng, z, ra, rb, s: (ra, [], []),                                           # an empty B row
    }
    s = System(nc, ni, seed=77, pool=400, special=special, unused=3, small_free=250)
    assert len({c for m in s.mats for r in m for c, _ in r}) > 300
    assert len(s.mats[0][700]) == 300 and len(s.mats[2][701]) == 200 and s.mats[1][704] == []
    assert z_full(s.z[s.mats[2][701][-1][1]]), "the 200-term row's own variable is not full-size"
    used = {col for m in s.mats for r in m for _, col in r}
    assert all(col not in used for col in range(len(s.z) - 3, len(s.z)))
    assert s.domain.size == 1 << 14
    handle = s.load(engine)
    keys = []
    try:
        wit, inst = _assignments([s.z], ni, dev)
        abc = torch.full((1, 3, nc, 4), -1, dtype=torch.int64, device=dev)
        bad = torch.full((1,), -1, dtype=torch.int32, device=dev)
        engine.r1cs_eval_dev(handle, 1, wit, inst, bad, abc, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        want = qap.matvec(s.mats, s.z)
        assert bad.tolist() == [0]
        for m in range(3):
            assert _canon(abc[0, m]) == want[m], "ABC"[m] + " z"
        h, badh = _witness_map(engine, handle, wit, inst)
        assert badh.tolist() == [0] and _canon(h[0]) == qap.witness_map(s.mats, ni, s.z)
        rng = random.Random(78)
        toxic = _toxic(rng)
        rs = [[rng.randrange(P), rng.randrange(P)]]
        proofs = []
        vk = None
        for mode in (eng_mod.KEY_TABLES, eng_mod.KEY_BARE):
            key, vk = _setup(engine, handle, toxic, mode=mode)
            keys.append(key)
            p, badp = _prove(engine, key, handle, wit, inst, rs)
            assert badp.tolist() == [0]
            proofs.append(p)
        assert torch.equal(proofs[0], proofs[1]), "the two kinds of key give different proofs"
        ver = frw.Groth16Verifier(vk)
        assert ver.verify(inst.cpu().numpy().view(np.uint64), proofs[0].cpu().numpy().view(np.uint64)).tolist() == [1]
        ver.close()
    finally:
        for k in keys:
            engine.groth16_pk_free(k)
        engine.r1cs_free(handle)


def z_full(v):
    return v >> 250 != 0


# ---- 5. the wire, on the 2^3 domain ----------------------------------------------------------------------------------------------------------
def test_wire_and_rerandomisation_on_the_2_3_domain(engine):
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    ni = 3
    s = System(5, ni, seed=55)
    assert s.domain.size == 8
    handle = s.load(engine)
    key = ver = None
    try:
        rng = random.Random(56)
        key, vk = _setup(engine, handle, _toxic(rng))
        wit, inst = _assignments([s.z], ni, dev)
        proofs, bad = _prove(engine, key, handle, wit, inst, [[rng.randrange(P), rng.randrange(P)]])
        assert bad.tolist() == [0]
        s0 = torch.cuda.current_stream().cuda_stream
        ver = frw.Groth16Verifier.from_wire(frw.vk_to_wire(vk), device=0)
        wire, st = frw.proofs_to_wire_dev(proofs, stream=s0)
        assert st.tolist() == [0]
        assert ver.verify_wire_dev(inst, wire.reshape(-1), stream=s0).tolist() == [1]
        wrong = inst.clone()
        wrong[0, 1] = _dev(_mont([(s.z[1] + 1) % P]), dev)[0]
        assert ver.verify_wire_dev(wrong, wire.reshape(-1), stream=s0).tolist() == [0]
        factors = _dev(T.ints_to_limbs([rng.randrange(1, P), rng.randrange(1, P)]).reshape(1, 2, 4), dev)
        fresh, st = ver.rerandomize_wire_dev(wire.reshape(-1), factors, stream=s0)
        assert st.tolist() == [0]
        assert ver.verify_wire_dev(inst, fresh.reshape(-1), stream=s0).tolist() == [1]
        old, new = wire.cpu().numpy()[0], fresh.cpu().numpy()[0]
        for lo, hi in ((0, 48), (48, 144), (144, 192)):
            assert old[lo:hi].tobytes() != new[lo:hi].tobytes(), "the re-randomised proof shares a point with its input"
    finally:
        if ver is not None:
            ver.close()
        if key is not None:
            engine.groth16_pk_free(key)
        engine.r1cs_free(handle)


# ---- 6. the example -----------------------------------------------------------------------------------------------------------------------
def test_the_example_exits_zero_with_both_lines():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "custom_r1cs.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True, timeout=300)
    assert res.returncode == 0, res.stdout
    lines = res.stdout.splitlines()
    assert "accepted: True" in lines and "accepted: False" in lines, res.stdout
    assert lines.index("accepted: True") < lines.index("accepted: False"), res.stdout
