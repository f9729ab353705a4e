"""The QAP witness map over a run-time modulus with a radix-2 domain (frw_qapf_*; falcon-r1cs_amd/csrc/frw_qap_field.hip).  Every
comparison is exact.  The shared system is a chain of squarings w_(i+1) = w_i^2 whose last value is public (I = 2: the constant one and
that value), in two shapes per domain 2^L: C = 2^L - 2 (the domain exactly full, the instance rows in the last slots) and
C = 2^(L-1) - 1 (one past the previous power: nearly half the domain is padding).
  1. over BLS12-381's r, L = 1 .. 17: byte for byte frw_qap_witness_map_dev, an unsatisfied statement included
  2. over bn254 (g = 5) and bls12_377 (g = 22), L = 1 .. 12 (13, 14 over bn254): the Python map of tests/qap_field_reference.py
  3. small two-adicity: 2^160+7 at n = 2, ed25519_l at n = 4, and its refusal of n = 8
  4. extreme operands   5. the Falcon-512 NTT circuit over bn254 (2^17), one slot refused   6. chunking   7. graph replay
  8. refusals   9. the example"""
import ctypes as C
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import field_cases as F
import frw_testlib as T
import qap_field_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERATOR = {"bn254": 5, "bls12_377": 22, "bls12_381": 7, "ed25519_l": 2, "2^160+7": 5}


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(torch.device("cuda:0"))


def _ints(t):
    return T.limbs_to_ints(t.cpu().numpy().view(np.uint64))


def _mont_dev(values, p, shape):
    return _dev(T.ints_to_limbs([F.mont(v % p, p) for v in values]).reshape(*shape, 4))


# ---- the chain of squarings -------------------------------------------------------------------------------------------------------------
def chain_csr(nc, ni, p):
    """rows i < C: w_i w_i = w_(i+1); the last value is instance variable 1 (I = 2) or one more witness variable (I = 1)"""
    ptr = np.arange(nc + 1, dtype=np.uint64)
    ab = np.arange(ni, ni + nc, dtype=np.uint32)
    c = ab + 1
    if ni == 2:
        c[-1] = 1
    one = np.tile(np.array(F.limbs4(1), dtype=np.uint64), (nc, 1))
    return [(ptr, ab, one), (ptr, ab, one), (ptr, c, one)], (nc if ni == 2 else nc + 1)


def chain_assignment(nc, ni, p, x, corrupt=None):
    """-> (instance values, witness values, A z, B z, C z), plain integers; corrupt: the witness element that gets + 1"""
    w = [x % p]
    for _ in range(nc):
        w.append(w[-1] * w[-1] % p)
    inst, wit = ([1, w[nc]], w[:nc]) if ni == 2 else ([1], w)
    if corrupt is not None:
        wit = list(wit)
        wit[corrupt] = (wit[corrupt] + 1) % p
    z = inst + wit
    az = [z[ni + i] for i in range(nc)]
    cz = [z[ni + i + 1] for i in range(nc - 1)] + [z[1] if ni == 2 else z[ni + nc]]
    return inst, wit, az, list(az), cz


def shapes(L):
    """(C, I) of the two shapes of the domain 2^L; with I = 2 the smallest domain is 2^2, so 2^1 is C = 1, I = 1"""
    if L == 1:
        return [(1, 1)]
    return [(nc, 2) for nc in sorted({(1 << L) - 2, (1 << (L - 1)) - 1}) if nc >= 1 and nc + 2 > (1 << (L - 1))]


def batch_of_three(nc, ni, p, seed):
    """three statements, statement 1 corrupted in one witness element -> device tensors and the plain assignments"""
    rng = random.Random(seed)
    plain = [chain_assignment(nc, ni, p, rng.randrange(2, p), corrupt=(nc // 2 if k == 1 else None)) for k in range(3)]
    inst = _mont_dev([v for s in plain for v in s[0]], p, (3, ni))
    wit = _mont_dev([v for s in plain for v in s[1]], p, (3, len(plain[0][1])))
    return inst, wit, plain


def witness_map(engine, q, wit, inst, statements_of_workspace=None, stream=None, out=None):
    """frw_qapf_witness_map_dev on device tensors -> (h, num), synchronised; the workspace is exactly what the call asks for"""
    import torch
    dev = torch.device("cuda:0")
    info = engine.qapf_info(q)
    batch = inst.shape[0]
    per = int(info.workspace_bytes_per_statement)
    size = per * (batch if statements_of_workspace is None else statements_of_workspace)
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    h = torch.full((batch, int(info.domain.size), 4), -1, dtype=torch.int64, device=dev) if out is None else out[0]
    num = torch.full((batch,), 12345, dtype=torch.int32, device=dev) if out is None else out[1]
    engine.qapf_witness_map_dev(q, batch, wit, inst, h, ws, size, num, torch.cuda.current_stream().cuda_stream if stream is None else stream)
    torch.cuda.synchronize()
    return h, num


def expected_h(p, g, plain):
    """the Python map of one statement, in Montgomery form"""
    inst, _, az, bz, cz = plain
    return [F.mont(v, p) for v in R.witness_map(p, g, az, bz, cz, inst)]


def unsatisfied(p, plain):
    return sum(1 for a, b, c in zip(*plain[2:]) if (a * b - c) % p)


# ---- 1. over r: device against device -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", range(1, 18))
def test_over_r_the_map_is_byte_for_byte_the_hard_wired_one(engine, L):
    import torch
    dev = torch.device("cuda:0")
    p = F.BLS12_381
    for nc, ni in shapes(L):
        mats, nw = chain_csr(nc, ni, p)
        inst, wit, plain = batch_of_three(nc, ni, p, 1000 + L)
        r = engine.r1cs_load_csr(ni, nw, mats)
        rf = engine.r1csf_load_csr(p, ni, nw, mats)
        q = engine.qapf_create(rf, 7)
        try:
            info = engine.qapf_info(q)
            assert (int(info.domain.log_size), int(info.num_constraints), int(info.num_instance)) == (L, nc, ni)
            qi = engine.qap_info(r)
            assert int(qi.domain_size) == 1 << L
            per = int(qi.workspace_bytes_per_signature)
            ws = torch.empty(3 * per, dtype=torch.uint8, device=dev)
            h_ref = torch.full((3, 1 << L, 4), -1, dtype=torch.int64, device=dev)
            num_ref = torch.full((3,), -1, dtype=torch.int32, device=dev)
            engine.qap_witness_map_dev(r, 3, wit, inst, h_ref, ws, 3 * per, num_ref, torch.cuda.current_stream().cuda_stream)
            h, num = witness_map(engine, q, wit, inst)
            assert num.tolist() == num_ref.tolist() == [unsatisfied(p, s) for s in plain]
            assert num.tolist()[0] == 0 and num.tolist()[1] >= 1
            assert torch.equal(h, h_ref), (L, nc)
        finally:
            engine.qapf_free(q)
            engine.r1csf_free(rf)
            engine.r1cs_free(r)


def test_the_domains_tested_over_r_include_the_first_of_every_pass_count(engine):
    """num_passes is 1 up to 2^12, 2 up to 2^16, 3 from 2^17 (frw_qap_field.h): the smallest L of each is among 1 .. 17"""
    import falcon_r1cs_amd as frw
    p = F.BLS12_381
    first = {}
    for L in range(1, 18):                                                    # the L of the test above, their first shape
        nc, ni = shapes(L)[0]
        mats, nw = chain_csr(nc, ni, p)
        rf = engine.r1csf_load_csr(p, ni, nw, mats)
        q = engine.qapf_create(rf, 7)
        try:
            first.setdefault(int(engine.qapf_info(q).num_passes), L)
        finally:
            engine.qapf_free(q)
            engine.r1csf_free(rf)
    assert first == {1: 1, 2: 13, 3: 17}
    assert frw.qapf_domain(p, 7, (1 << 22) - 2, 2).log_size == 22            # the largest domain is still three passes: 8 + 7 + 7


# ---- 2. against Python -----------------------------------------------------------------------------------------------------------------
def assert_equals_python(engine, name, nc, ni, seed):
    p, g = F.MODULI[name], GENERATOR[name]
    mats, nw = chain_csr(nc, ni, p)
    inst, wit, plain = batch_of_three(nc, ni, p, seed)
    rf = engine.r1csf_load_csr(p, ni, nw, mats)
    q = engine.qapf_create(rf, g)
    try:
        h, num = witness_map(engine, q, wit, inst)
        assert num.tolist() == [unsatisfied(p, s) for s in plain] and num.tolist()[1] >= 1
        for k in range(3):
            assert _ints(h[k]) == expected_h(p, g, plain[k]), (name, nc, k)
    finally:
        engine.qapf_free(q)
        engine.r1csf_free(rf)


@pytest.mark.parametrize("L", range(1, 13))
@pytest.mark.parametrize("name", ["bn254", "bls12_377"])
def test_against_the_python_map(engine, name, L):
    for nc, ni in shapes(L):
        assert_equals_python(engine, name, nc, ni, 2000 + L)


@pytest.mark.parametrize("L", [13, 14])
def test_two_passes_against_the_python_map_over_bn254(engine, L):
    assert_equals_python(engine, "bn254", (1 << L) - 2, 2, 2000 + L)


# ---- 3. small two-adicity ---------------------------------------------------------------------------------------------------------------
def test_a_field_of_two_adicity_one_has_the_domain_of_two_points(engine):
    assert_equals_python(engine, "2^160+7", 1, 1, 31)


def test_a_field_of_two_adicity_two_has_the_domain_of_four_points_and_no_larger(engine):
    import falcon_r1cs_amd as frw
    assert_equals_python(engine, "ed25519_l", 2, 2, 32)
    assert_equals_python(engine, "ed25519_l", 1, 2, 33)
    p = F.ED25519_L
    ONE, Y, X, X2, X3 = range(5)
    cubic = ([[(X, 1)], [(X2, 1)], [(X3, 1), (X, 1), (ONE, 5)]], [[(X, 1)], [(X, 1)], [(ONE, 1)]], [[(X2, 1)], [(X3, 1)], [(Y, 1)]])
    mats = [(np.array([0] + list(np.cumsum([len(r) for r in m])), dtype=np.uint64), np.array([c for r in m for c, _ in r], dtype=np.uint32),
             np.array([F.limbs4(v % p) for r in m for _, v in r], dtype=np.uint64).reshape(-1, 4)) for m in cubic]
    rf = engine.r1csf_load_csr(p, 2, 3, mats)                                # C + I = 5: 2^3 > 2^2
    try:
        with pytest.raises(frw.FrwError) as err:
            engine.qapf_create(rf, 2)
        assert err.value.code == -1 and "PolynomialDegreeTooLarge" in str(err.value)
    finally:
        engine.r1csf_free(rf)


# ---- 4. extreme operands ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bn254", "bls12_377"])
def test_extreme_operands(engine, name):
    """n = 8: every row of A z, B z and C z is p - 1, then p - 2 (row i of all three matrices reads w_i, every variable that value)"""
    p, g = F.MODULI[name], GENERATOR[name]
    nc, ni = 6, 2
    ptr = np.arange(nc + 1, dtype=np.uint64)
    col = np.arange(ni, ni + nc, dtype=np.uint32)
    one = np.tile(np.array(F.limbs4(1), dtype=np.uint64), (nc, 1))
    rf = engine.r1csf_load_csr(p, ni, nc, [(ptr, col, one)] * 3)
    q = engine.qapf_create(rf, g)
    try:
        for v in (p - 1, p - 2):
            inst = _mont_dev([1, v], p, (1, ni))
            wit = _mont_dev([v] * nc, p, (1, nc))
            h, num = witness_map(engine, q, wit, inst)
            assert num.tolist() == [nc if (v * v - v) % p else 0]
            assert _ints(h[0]) == [F.mont(x, p) for x in R.witness_map(p, g, [v] * nc, [v] * nc, [v] * nc, [1, v])]
    finally:
        engine.qapf_free(q)
        engine.r1csf_free(rf)


# ---- 5. the Falcon-512 NTT circuit over bn254 ----------------------------------------------------------------------------------------------
def test_falcon_512_over_bn254(engine):
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    p, g, logn = F.BN254, 5, 9
    rng = random.Random(5)
    good, bad = T.random_triple(logn, rng), T.random_triple(logn, rng)
    bad[0][100] = F.Q                                                          # a coefficient >= q: refused, zero-filled
    L = frw.layout(logn)
    sig, pk, hm = (np.stack([t[k] for t in (good, bad)]) for k in range(3))
    wit = torch.full((2, L.num_witness, 4), -1, dtype=torch.int64, device=dev)
    inst = torch.full((2, L.num_instance, 4), -1, dtype=torch.int64, device=dev)
    st = torch.full((2,), -7, dtype=torch.int32, device=dev)
    as_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(dev)
    engine.witness_ntt_verify_dev(logn, 2, as_dev(sig), as_dev(pk), as_dev(hm), wit, inst, st, engine.field_encoding(p),
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st.tolist() == [frw.ST_OK, frw.ST_COEFF_RANGE]
    rf = engine.r1csf_load(0, logn, p)
    q = engine.qapf_create(rf, g)
    try:
        info = engine.qapf_info(q)
        nc, ni, n = int(info.num_constraints), int(info.num_instance), int(info.domain.size)
        assert (n, int(info.num_passes)) == (1 << 17, 3)
        h, num = witness_map(engine, q, wit, inst)
        assert [v & 0xFFFFFFFF for v in num.tolist()] == [0, nc]
        assert not h[1].any()                                                  # the refused slot: all zero
        abc = torch.empty((1, 3, nc, 4), dtype=torch.int64, device=dev)
        need = engine.r1csf_scratch_bytes(rf, 1, True)
        scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        cnt = torch.empty(1, dtype=torch.int32, device=dev)
        engine.r1csf_check_dev(rf, 1, wit, inst, cnt, None, abc, scratch, need, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        rinv = pow(1 << 256, -1, p)
        az, bz, cz = ([v * rinv % p for v in _ints(abc[0, m])] for m in range(3))
        inputs = [v * rinv % p for v in _ints(inst[0])]
        hh = [v * rinv % p for v in _ints(h[0])]
        assert inputs[0] == 1 and hh[n - 1] == 0
        for _ in range(2):
            lhs, rhs = R.check_identity(p, g, az, bz, cz, inputs, hh, rng.randrange(2, p))
            assert lhs == rhs
    finally:
        engine.qapf_free(q)
        engine.r1csf_free(rf)


# ---- 6. chunking, 7. graph replay, 8. refusals ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def two_pass_statements(batch):
    """a two-pass domain (2^13, the padded shape) over bn254: the system and `batch` statements, the second one corrupted"""
    p, nc, ni = F.BN254, (1 << 12) - 1, 2
    rng = random.Random(6)
    plain = [chain_assignment(nc, ni, p, rng.randrange(2, p), corrupt=(7 if k == 1 else None)) for k in range(batch)]
    return p, nc, ni, plain


def test_a_workspace_of_two_statements_serves_a_batch_of_five(engine):
    import torch
    p, nc, ni, plain = two_pass_statements(5)
    mats, nw = chain_csr(nc, ni, p)
    inst = _mont_dev([v for s in plain for v in s[0]], p, (5, ni))
    wit = _mont_dev([v for s in plain for v in s[1]], p, (5, nw))
    rf = engine.r1csf_load_csr(p, ni, nw, mats)
    q = engine.qapf_create(rf, 5)
    try:
        h_all, num_all = witness_map(engine, q, wit, inst)
        h_two, num_two = witness_map(engine, q, wit, inst, statements_of_workspace=2)
        assert num_all.tolist() == num_two.tolist() == [unsatisfied(p, s) for s in plain]
        assert torch.equal(h_all, h_two)
        assert _ints(h_two[4]) == expected_h(p, 5, plain[4])
    finally:
        engine.qapf_free(q)
        engine.r1csf_free(rf)


def test_the_call_is_captured_and_replays_on_a_changed_witness(engine):
    import torch
    dev = torch.device("cuda:0")
    p, nc, ni, plain = two_pass_statements(2)
    mats, nw = chain_csr(nc, ni, p)
    rf = engine.r1csf_load_csr(p, ni, nw, mats)
    q = engine.qapf_create(rf, 5)
    try:
        info = engine.qapf_info(q)
        per = int(info.workspace_bytes_per_statement)
        inst = _mont_dev(plain[0][0], p, (1, ni))
        wit = _mont_dev(plain[0][1], p, (1, nw))
        ws = torch.empty(per, dtype=torch.uint8, device=dev)
        h = torch.zeros((1, int(info.domain.size), 4), dtype=torch.int64, device=dev)
        num = torch.zeros(1, dtype=torch.int32, device=dev)
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            engine.qapf_witness_map_dev(q, 1, wit, inst, h, ws, per, num, side.cuda_stream)
        for s in (plain[0], plain[1]):
            inst.copy_(_mont_dev(s[0], p, (1, ni)))
            wit.copy_(_mont_dev(s[1], p, (1, nw)))
            h.fill_(-1)
            num.fill_(99)
            graph.replay()
            torch.cuda.synchronize()
            h_direct, num_direct = witness_map(engine, q, wit, inst)
            assert num.tolist() == num_direct.tolist() == [unsatisfied(p, s)]
            assert torch.equal(h, h_direct)
        assert unsatisfied(p, plain[0]) == 0 and unsatisfied(p, plain[1]) >= 1
    finally:
        engine.qapf_free(q)
        engine.r1csf_free(rf)


def test_refusals(engine):
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    lib = frw.load_library()
    p, nc, ni = F.BN254, 6, 2
    mats, nw = chain_csr(nc, ni, p)
    s = chain_assignment(nc, ni, p, 3)
    inst, wit = _mont_dev(s[0], p, (1, ni)), _mont_dev(s[1], p, (1, nw))
    rf = engine.r1csf_load_csr(p, ni, nw, mats)
    q = engine.qapf_create(rf, 5)
    try:
        per = int(engine.qapf_info(q).workspace_bytes_per_statement)
        ws = torch.empty(per + 16, dtype=torch.uint8, device=dev)
        h = torch.full((1, 8, 4), 77, dtype=torch.int64, device=dev)
        num = torch.full((1,), 77, dtype=torch.int32, device=dev)
        P = lambda t: C.c_void_p(t.data_ptr())
        call = lambda qq, b, w, i, hh, n, s_, sb: lib.frw_qapf_witness_map_dev(qq, b, w, i, hh, n, s_, sb, None)
        assert call(None, 1, P(wit), P(inst), P(h), P(num), P(ws), per) == -1
        assert call(q, 1, None, P(inst), P(h), P(num), P(ws), per) == -1
        assert call(q, 1, P(wit), None, P(h), P(num), P(ws), per) == -1
        assert call(q, 1, P(wit), P(inst), None, P(num), P(ws), per) == -1
        assert call(q, 1, P(wit), P(inst), P(h), P(num), None, per) == -1
        assert call(q, 1, P(wit), P(inst), P(h), P(num), P(ws), per - 1) == -1                 # one byte short of a statement
        assert call(q, 0, None, None, None, None, None, 0) == 0                                # batch = 0 touches nothing
        assert call(None, 0, None, None, None, None, None, 0) == 0
        torch.cuda.synchronize()
        assert num.tolist() == [77] and h.eq(77).all()
        assert call(q, 1, P(wit), P(inst), P(h), None, P(ws), per) == 0                        # d_num_unsatisfied may be NULL
        torch.cuda.synchronize()
        assert num.tolist() == [77] and _ints(h[0]) == expected_h(p, 5, s)
        assert lib.frw_qapf_info(None, None) == -1 and lib.frw_qapf_create(None, None, None) == -1
        out = C.c_void_p(1)
        assert lib.frw_qapf_create(rf, None, C.byref(out)) == -1 and not out.value
        with pytest.raises(frw.FrwError):
            engine.qapf_create(rf, 4)                                                          # a square
    finally:
        engine.qapf_free(q)
        engine.r1csf_free(rf)
    engine.qapf_free(None)


# ---- 9. the example ----------------------------------------------------------------------------------------------------------------------
def test_the_example_exits_zero():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "witness_map_bn254.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True, timeout=300)
    assert res.returncode == 0, res.stdout
