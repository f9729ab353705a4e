"""The satisfaction check and A z, B z, C z over a run-time modulus (frw_r1csf_check_dev; falcon-r1cs_amd/csrc/frw_r1cs_field.hip).
Every expectation is Python integers: matrices applied to the bytes read back, mod p.
  1. the example system x^3 + x + 5 = y over four moduli: satisfied / one row violated / instance[0] = 0, batch 3 and batch 130
  2. extreme operands (every coefficient and variable p - 1, then p - 2) and the row shapes around the long-row threshold
  3. the Falcon-512 NTT circuit over bn254 and 2^160+7 on witnesses the device wrote under the field encoding, against the
     oracle's matrices over p
  4. Falcon-1024 over bn254 (the 160-bit coefficients)
  5. BLS12-381's modulus through the new handle == frw_r1cs_check_dev / frw_r1cs_eval_dev, byte for byte
  6. the dual circuit over bn254 on the oracle's witness
  7. graph replay   8. refusals   9. the example"""
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

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
LONG_ROW = 64               # R1CSF_LONG_ROW of frw_r1cs_field.h: rows from here on take a wavefront


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(torch.device("cuda:0"))


def _ints(t):
    return T.limbs_to_ints(t.cpu().numpy().view(np.uint64))


def _mont_dev(values, p, shape):
    """integers -> x 2^256 mod p as an int64 device tensor of `shape` + (4,)"""
    return _dev(T.ints_to_limbs([F.mont(v % p, p) for v in values]).reshape(*shape, 4))


def reference(mats, ni, z_inst, z_wit, p):
    """mats: A, B, C as lists of rows of (column, coefficient); the vectors canonical -> (violated rows, first or NONE, [Az, Bz, Cz])"""
    if z_inst[0] != 1:
        nc = len(mats[0])
        return nc, 0, [[0] * nc for _ in range(3)]
    z = list(z_inst) + list(z_wit)
    assert len(z_inst) == ni
    abc = [[sum(c * z[col] for col, c in row) % p for row in m] for m in mats]
    bad = [i for i, (a, b, c) in enumerate(zip(*abc)) if (a * b - c) % p]
    return len(bad), (bad[0] if bad else NONE), abc


def check(engine, handle, wit, inst, with_abc, first=True, stream=None):
    """frw_r1csf_check_dev on device tensors -> (num, first, abc) tensors, synchronised; the scratch is exactly what the call asks for"""
    import torch
    dev = torch.device("cuda:0")
    batch = inst.shape[0]
    info = engine.r1csf_info(handle)
    num = torch.full((batch,), 12345, dtype=torch.int32, device=dev)
    fst = torch.full((batch,), 12345, dtype=torch.int32, device=dev) if first else None
    abc = torch.full((batch, 3, int(info.num_constraints), 4), -1, dtype=torch.int64, device=dev) if with_abc else None
    need = engine.r1csf_scratch_bytes(handle, batch, with_abc)
    assert need == batch * int(info.scratch_bytes_per_statement[1 if with_abc else 0])
    scratch = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    engine.r1csf_check_dev(handle, batch, wit, inst, num, fst, abc, scratch, need,
                           torch.cuda.current_stream().cuda_stream if stream is None else stream)
    torch.cuda.synchronize()
    return num, fst, abc


def u32(t):
    return [v & 0xFFFFFFFF for v in t.tolist()]


def assert_matches(engine, handle, wit, inst, mats, p, statements=None, abc_for=None):
    """both forms of the call against the reference, for the statements named (default: all)"""
    batch = inst.shape[0]
    ni = inst.shape[1]
    rinv = pow(1 << 256, -1, p)
    statements = range(batch) if statements is None else statements
    want = {}
    for k in statements:
        zi, zw = [v * rinv % p for v in _ints(inst[k])], [v * rinv % p for v in _ints(wit[k])]
        want[k] = reference(mats, ni, zi, zw, p)
    n1, f1, abc = check(engine, handle, wit, inst, True)
    n0, f0, _ = check(engine, handle, wit, inst, False)
    n2, _, _ = check(engine, handle, wit, inst, False, first=False)           # d_first_unsatisfied = NULL
    assert u32(n1) == u32(n0) == u32(n2) and u32(f1) == u32(f0)
    got_n, got_f = u32(n1), u32(f1)
    for k in statements:
        assert (got_n[k], got_f[k]) == want[k][:2], k
    for k in (statements if abc_for is None else abc_for):
        flat = [F.mont(v, p) for m in want[k][2] for v in m]
        assert _ints(abc[k].reshape(-1, 4)) == flat, k
    return want


# ---- 1. the example system ----------------------------------------------------------------------------------------------------------------
ONE, Y, X, X2, X3 = range(5)
CUBIC = ([[(X, 1)], [(X2, 1)], [(X3, 1), (X, 1), (ONE, 5)]], [[(X, 1)], [(X, 1)], [(ONE, 1)]], [[(X2, 1)], [(X3, 1)], [(Y, 1)]])


def csr(mats, p):
    return [(np.array([0] + list(np.cumsum([len(r) for r in m])), dtype=np.uint64), np.array([c for r in m for c, _ in r], dtype=np.uint32),
             np.array([F.limbs4(v % p) for r in m for _, v in r], dtype=np.uint64).reshape(-1, 4)) for m in mats]


@pytest.mark.parametrize("name", ["bn254", "2^255-19", "2^160+7", "bls12_377"])
def test_the_example_system(engine, name):
    p = F.MODULI[name]
    h = engine.r1csf_load_csr(p, 2, 3, csr(CUBIC, p))
    try:
        info = engine.r1csf_info(h)
        assert (int(info.num_instance), int(info.num_witness), int(info.num_constraints), list(info.nnz)) == (2, 3, 3, [5, 3, 3])
        assert sum(int(v) << (64 * i) for i, v in enumerate(info.modulus)) == p
        assert list(info.scratch_bytes_per_statement) == [0, 0]               # no long row: no scratch, NULL is taken
        x = p - 3                                                             # x^3 wraps the modulus many times over
        y = (x ** 3 + x + 5) % p
        kinds = [([1, y], [x, x * x, x ** 3]),                                 # satisfied
                 ([1, y], [x, x * x + 1, x ** 3]),                             # x2 is wrong: rows 0 and 1
                 ([0, y], [x, x * x, x ** 3])]                                 # no leading one
        for batch in (3, 130):                                                # 130: more than two wavefronts of statements
            inst = _mont_dev([v for k in range(batch) for v in kinds[k % 3][0]], p, (batch, 2))
            wit = _mont_dev([v for k in range(batch) for v in kinds[k % 3][1]], p, (batch, 3))
            want = assert_matches(engine, h, wit, inst, CUBIC, p)
            assert [want[k][:2] for k in range(3)] == [(0, NONE), (2, 0), (3, 0)]
    finally:
        engine.r1csf_free(h)


# ---- 2. extreme operands, row shapes --------------------------------------------------------------------------------------------------
def shapes_system(p, coef):
    """I = 2, W = 200 (witness 199 unused).  Rows of T - 1, T, T + 1 and 2 * 64 + 1 terms in A (and the T-term one in C as well, the
    129-term one in B), a row with a column three times and a zero coefficient, an empty row -- every other coefficient `coef`."""
    ni = 2
    w = lambda k: ni + k
    a, b, c = [], [], []
    for n in (LONG_ROW - 1, LONG_ROW, LONG_ROW + 1, 2 * 64 + 1):
        a.append([(w(k), coef) for k in range(n)])
        b.append([(w(k + 3), coef) for k in range(n)] if n == 129 else [(ONE, coef)])
        c.append([(w(2 * k % 199), coef) for k in range(n)] if n == LONG_ROW else [(1, coef), (w(7), coef)])
    a.append([(w(5), coef), (w(5), coef), (w(6), 0), (w(5), coef)]); b.append([(ONE, 1)]); c.append([(w(5), coef), (w(5), (2 * coef) % p)])   # satisfied: 3 c z = c z + 2 c z
    a.append([]); b.append([(w(1), coef)]); c.append([])                                                                                  # satisfied: 0 * b = 0
    a.append([(w(0), coef)]); b.append([]); c.append([(ONE, coef)])                                                                        # violated: 0 != c
    return a, b, c


@pytest.mark.parametrize("name", ["2^255-19", "bn254"])
def test_extreme_operands_and_row_shapes(engine, name):
    p = F.MODULI[name]
    for coef in (p - 1, p - 2):                                               # p - 1 is the class "-1" (no product); p - 2 takes the product
        mats = shapes_system(p, coef)
        h = engine.r1csf_load_csr(p, 2, 200, csr(mats, p))
        try:
            info = engine.r1csf_info(h)
            assert int(info.num_constraints) == 7
            # long: A rows 1, 2, 3; B row 3; C row 1 -- check only, their five products wait in the scratch; either way it holds the plain
            # values of the variables they read (the constant and witnesses 0 .. 131: 133 of them), four bytes apiece, in whole 32-byte lines
            per = list(info.scratch_bytes_per_statement)
            assert per[0] - per[1] == 5 * 32 and per[1] == 136 * 4
            rng = random.Random(coef % 1000)
            vecs = [([1, p - 1], [p - 1] * 200), ([1, 0], [0] * 200), ([1, rng.randrange(p)], [rng.randrange(p) for _ in range(200)]),
                    ([1, p - 1], [p - 1] * 200), ([1, 1], [1] * 200),
                    ([1, 5], [(1 << 32) - 1 - (k & 1) for k in range(200)])]         # the largest plain values the long rows take as they are
            # (six: a ragged group of the long-row kernel; variables that are small integers and variables that are not, in one row too)
            inst = _mont_dev([v for zi, _ in vecs for v in zi], p, (6, 2))
            wit = _mont_dev([v for _, zw in vecs for v in zw], p, (6, 200))
            want = assert_matches(engine, h, wit, inst, mats, p)
            assert all(0 < want[k][0] < 7 for k in (0, 2))                    # the rows made to hold do, the one made to fail does not
        finally:
            engine.r1csf_free(h)


# ---- Falcon circuits ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_system(circuit, name, logn=9):
    """the oracle's constraint system over the modulus, built once: (matrices as rows of (column, coefficient), the system itself)"""
    from oracle import falcon_gadgets as G
    from oracle.ark_sim import ConstraintSystem
    sig, pk, hm, _ = T.random_triple(logn, random.Random(41))
    cs = ConstraintSystem(F.MODULI[name])
    cls = G.FalconDualNTTVerificationCircuit if circuit else G.FalconNTTVerificationCircuit
    cls(sig.tolist(), pk.tolist(), hm.tolist(), logn).generate_constraints(cs)
    return cs.to_matrices(), cs


def falcon_witness(engine, logn, triples, enc):
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    L = frw.layout(logn)
    sig, pk, hm = (np.stack([t[k] for t in triples]) for k in range(3))
    batch = len(triples)
    wit = torch.full((batch, L.num_witness, 4), -1, dtype=torch.int64, device=dev)
    inst = torch.full((batch, L.num_instance, 4), -1, dtype=torch.int64, device=dev)
    st = torch.full((batch,), -7, dtype=torch.int32, device=dev)
    engine.witness_ntt_verify_dev(logn, batch, _dev(sig), _dev(pk), _dev(hm), wit, inst, st, enc, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return wit, inst, st


@pytest.mark.parametrize("name", ["bn254", "2^160+7"])
def test_falcon_512_against_the_oracles_matrices_over_p(engine, name):
    import falcon_r1cs_amd as frw
    p, logn = F.MODULI[name], 9
    mats, _ = oracle_system(0, name)
    rng = random.Random(3)
    good, other, loud = T.random_triple(logn, rng), T.random_triple(logn, rng), T.random_triple(logn, rng, scale=1.6)
    wit, inst, st = falcon_witness(engine, logn, [good, other, loud], engine.field_encoding(p))
    assert st.tolist() == [frw.ST_OK, frw.ST_OK, frw.ST_NORM_BOUND]           # permissive: the third is written, and unsatisfied
    wit[1, 40000, 0] += 1                                                     # one witness element, on the device
    h = engine.r1csf_load(0, logn, p)
    try:
        info = engine.r1csf_info(h)
        assert [len(m) for m in mats] == [int(info.num_constraints)] * 3 and [sum(len(r) for r in m) for m in mats] == list(info.nnz)
        want = assert_matches(engine, h, wit, inst, mats, p, abc_for=[1])
        assert want[0][:2] == (0, NONE) and want[1][0] >= 1 and want[2][0] >= 1
    finally:
        engine.r1csf_free(h)


def test_falcon_1024_over_bn254(engine):
    p, logn = F.BN254, 10
    wit, inst, st = falcon_witness(engine, logn, [T.random_triple(logn, random.Random(10))], engine.field_encoding(p))
    assert st.tolist() == [0]
    h = engine.r1csf_load(0, logn, p)
    try:
        num, fst, _ = check(engine, h, wit, inst, False)
        assert (u32(num), u32(fst)) == ([0], [NONE])
        wit[0, 123456, 1] ^= 1                                                # one flipped bit of one element
        num, fst, _ = check(engine, h, wit, inst, False)
        assert u32(num)[0] >= 1 and u32(fst)[0] < 162870
        num2, fst2, _ = check(engine, h, wit, inst, True)
        assert u32(num2) == u32(num) and u32(fst2) == u32(fst)
    finally:
        engine.r1csf_free(h)


def test_bls12_381_through_the_new_handle_equals_the_hard_wired_path(engine):
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    logn = 9
    rng = random.Random(381)
    wit, inst, st = falcon_witness(engine, logn, [T.random_triple(logn, rng), T.random_triple(logn, rng)], frw.ENC_MONTGOMERY)
    assert st.tolist() == [0, 0]
    wit[1, 777, 0] += 1
    r = engine.r1cs_load(0, logn)
    h = engine.r1csf_load(0, logn, F.BLS12_381)
    try:
        nc = frw.layout(logn).num_constraints
        bad_eval, bad_check = (torch.full((2,), -1, dtype=torch.int32, device=dev) for _ in range(2))
        abc_ref = torch.full((2, 3, nc, 4), -1, dtype=torch.int64, device=dev)
        engine.r1cs_eval_dev(r, 2, wit, inst, bad_eval, abc_ref)
        engine.r1cs_check_dev(r, 2, wit, inst, bad_check)
        torch.cuda.synchronize()
        num, _, abc = check(engine, h, wit, inst, True)
        num0, _, _ = check(engine, h, wit, inst, False)
        assert num.tolist() == num0.tolist() == bad_eval.tolist() == bad_check.tolist()
        assert num.tolist()[0] == 0 and num.tolist()[1] >= 1
        assert torch.equal(abc, abc_ref)
    finally:
        engine.r1csf_free(h)
        engine.r1cs_free(r)


def test_dual_circuit_over_bn254_on_the_oracles_witness(engine):
    p, name = F.BN254, "bn254"
    _, cs = oracle_system(1, name)
    assert cs.is_satisfied()
    inst = _mont_dev(cs.instance_assignment, p, (1, cs.num_instance_variables()))
    wit = _mont_dev(cs.witness_assignment, p, (1, cs.num_witness_variables()))
    h = engine.r1csf_load(1, 9, p)
    try:
        info = engine.r1csf_info(h)
        assert (int(info.num_instance), int(info.num_witness), int(info.num_constraints)) == (
            cs.num_instance_variables(), cs.num_witness_variables(), cs.num_constraints())
        num, fst, _ = check(engine, h, wit, inst, False)
        assert (u32(num), u32(fst)) == ([0], [NONE])
        wit[0, 5000, 0] ^= 2
        num, fst, _ = check(engine, h, wit, inst, True)
        assert u32(num)[0] >= 1 and u32(fst)[0] < cs.num_constraints()
    finally:
        engine.r1csf_free(h)


# ---- 7. graph replay ---------------------------------------------------------------------------------------------------------------------
def test_the_call_is_captured_and_replays_on_what_the_buffers_hold(engine):
    import torch
    dev = torch.device("cuda:0")
    p = F.BN254
    mats = shapes_system(p, p - 2)                                            # long rows: the scratch is part of the capture
    h = engine.r1csf_load_csr(p, 2, 200, csr(mats, p))
    try:
        rng = random.Random(7)
        first = ([1, 5], [rng.randrange(p) for _ in range(200)])
        second = ([1, 5], [0] * 200)
        rinv = pow(1 << 256, -1, p)
        inst = _mont_dev(first[0], p, (1, 2))
        wit = _mont_dev(first[1], p, (1, 200))
        num = torch.zeros(1, dtype=torch.int32, device=dev)
        fst = torch.zeros(1, dtype=torch.int32, device=dev)
        need = engine.r1csf_scratch_bytes(h, 1, False)
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            engine.r1csf_check_dev(h, 1, wit, inst, num, fst, None, scratch, need, side.cuda_stream)
        for zi, zw in (first, second):
            wit.copy_(_mont_dev(zw, p, (1, 200)))
            num.fill_(99)
            fst.fill_(99)
            graph.replay()
            torch.cuda.synchronize()
            want = reference(mats, 2, zi, zw, p)
            assert (u32(num)[0], u32(fst)[0]) == want[:2]
        assert reference(mats, 2, *first, p)[:2] != reference(mats, 2, *second, p)[:2]
        del rinv
    finally:
        engine.r1csf_free(h)


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(engine):
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    lib = frw.load_library()
    p = F.BN254
    mats = shapes_system(p, p - 2)
    h = engine.r1csf_load_csr(p, 2, 200, csr(mats, p))
    try:
        inst = _mont_dev([1, 5], p, (1, 2))
        wit = _mont_dev([3] * 200, p, (1, 200))
        num = torch.full((1,), 77, dtype=torch.int32, device=dev)
        need = engine.r1csf_scratch_bytes(h, 1, False)
        need_abc = engine.r1csf_scratch_bytes(h, 1, True)
        assert need - need_abc == 5 * 32 and need_abc > 0
        scratch = torch.empty(need + 16, dtype=torch.uint8, device=dev)
        P = lambda t: C.c_void_p(t.data_ptr())
        call = lambda hh, b, w, i, n, s, sb: lib.frw_r1csf_check_dev(hh, b, w, i, n, None, None, s, sb, None)
        assert call(None, 1, P(wit), P(inst), P(num), P(scratch), need) == -1
        assert call(h, 1, None, P(inst), P(num), P(scratch), need) == -1
        assert call(h, 1, P(wit), None, P(num), P(scratch), need) == -1
        assert call(h, 1, P(wit), P(inst), None, P(scratch), need) == -1
        assert call(h, 1, P(wit), P(inst), P(num), None, need) == -1
        assert call(h, 1, P(wit), P(inst), P(num), P(scratch), need - 1) == -1
        assert call(h, 1, P(wit), P(inst), P(num), C.c_void_p(scratch.data_ptr() + 8), need) == -1       # misaligned
        assert call(h, 0, None, None, None, None, 0) == 0                      # batch = 0 touches nothing
        assert call(None, 0, None, None, None, None, 0) == 0
        torch.cuda.synchronize()
        assert num.tolist() == [77]
        # with products the long rows' results need no scratch, the plain values of their variables do
        abc = torch.empty((1, 3, 7, 4), dtype=torch.int64, device=dev)
        assert lib.frw_r1csf_check_dev(h, 1, P(wit), P(inst), P(num), None, P(abc), None, 0, None) == -1
        assert lib.frw_r1csf_check_dev(h, 1, P(wit), P(inst), P(num), None, P(abc), P(scratch), need_abc - 1, None) == -1
        torch.cuda.synchronize()
        assert num.tolist() == [77]
        assert lib.frw_r1csf_check_dev(h, 1, P(wit), P(inst), P(num), None, P(abc), P(scratch), need_abc, None) == 0
        torch.cuda.synchronize()
        assert num.tolist() != [77]
        with pytest.raises(frw.FrwError):
            engine.r1csf_load(0, 9, F.REFUSED["even"])
        with pytest.raises(frw.FrwError):
            engine.r1csf_load_csr(p, 2, 3, csr(([[(X, p)]], [[(X, 1)]], [[(X, 1)]]), 1 << 255))           # a value >= p
    finally:
        engine.r1csf_free(h)
    engine.r1csf_free(None)


def test_a_file_loads_like_the_arrays(engine, tmp_path):
    import falcon_r1cs_amd as frw
    p = F.BLS12_377
    path = tmp_path / "dual9.r1cs"
    counts = frw.r1cs_export_field(1, 9, p, path)
    h = engine.r1csf_load_file(p, path)
    try:
        info = engine.r1csf_info(h)
        assert [int(info.num_instance), int(info.num_witness), int(info.num_constraints)] + list(info.nnz) == counts
    finally:
        engine.r1csf_free(h)


# ---- 9. the example ----------------------------------------------------------------------------------------------------------------------
def test_the_example_exits_zero():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "is_satisfied_bn254.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True, timeout=300)
    assert res.returncode == 0, res.stdout
    assert "violated rows: 0" in res.stdout, res.stdout
