"""frw_groth16_rerandomize (host code, falcon-r1cs_amd/csrc/frw_rerand.h) against oracle/bls12_381.py, bit for bit: the case list of
tests/rerandomize_cases.py -- random factors, factors >= r, every multiplier (r1^-1, r1, r2, r1 r2) at the edge values of the split by
lambda, points at infinity, equal and opposite summands in B' and C', zero factors, malformed proofs with and without the vouching
flag -- then in place, independence of the batch, and the oracle's verify_proof on a re-randomised proof of a real statement."""
import numpy as np
import pytest

import falcon_r1cs_amd as frw
import rerandomize_cases as RC
from oracle import bls12_381 as E


@pytest.fixture(scope="module")
def env(oracle):
    cs = RC.build(oracle)
    ver = frw.Groth16Verifier(cs.key.limbs())
    yield cs, ver
    ver.close()


@pytest.mark.parametrize("vouched", [False, True])
def test_the_case_list_equals_the_oracle(env, vouched):
    cs, ver = env
    flags = frw.VERIFY_POINTS_ARE_CHECKED if vouched else 0
    out, status = ver.rerandomize(cs.proofs(), cs.factors(), flags)
    RC.check(cs, out, status, vouched)
    names = [c.name for c in cs.cases]
    assert out[names.index("five")].tolist() == out[names.index("r-plus-five")].tolist()      # r + 5 gives what 5 gives
    # deterministic, also where the result is unspecified
    again, status2 = ver.rerandomize(cs.proofs(), cs.factors(), flags)
    assert again.tolist() == out.tolist() and status2.tolist() == status.tolist()


def test_in_place_and_one_at_a_time(env):
    cs, ver = env
    proofs, factors = cs.proofs(), cs.factors()
    want, want_status = ver.rerandomize(proofs, factors)
    lib = frw.load_library()
    buf = proofs.copy()
    status = np.full(len(buf), 9, dtype=np.int32)
    import ctypes as C
    v = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.frw_groth16_rerandomize(ver._h, len(buf), v(buf), v(factors), 0, v(buf), v(status)) == 0
    assert buf.tolist() == want.tolist() and status.tolist() == want_status.tolist()
    # a slot's output depends on its own proof and factors alone
    for i in (0, 7, len(proofs) - 1):
        one, st = ver.rerandomize(proofs[i:i + 1], factors[i:i + 1])
        assert one[0].tolist() == want[i].tolist() and st[0] == want_status[i]


def test_a_rerandomised_proof_verifies_for_its_statement_alone(env):
    cs, ver = env
    c = cs.cases[0]
    assert c.name == "random-valid"
    out, status = ver.rerandomize(c.proof[None], c.factors[None])
    assert status[0] == 0
    proof = (E.from_limbs(out[0, :12]), E.g2_from_limbs(out[0, 12:36]), E.from_limbs(out[0, 36:]))
    assert all(proof[i] != cs.valid_proof[i] for i in range(3))                                  # a new proof in every point
    vk = cs.vk_dict()
    assert E.verify_proof(vk, cs.statement, cs.valid_proof)
    assert E.verify_proof(vk, cs.statement, proof)
    assert not E.verify_proof(vk, [cs.statement[0], (cs.statement[1] + 1) % E.R], proof)
    # the product's own verifier agrees (instance vector: the constant one first, canonical encoding)
    import frw_testlib as T
    inst = T.ints_to_limbs([1] + cs.statement)[None]
    assert ver.verify(inst, out, frw.ENC_CANONICAL).tolist() == [1]
    inst2 = T.ints_to_limbs([1, cs.statement[0], (cs.statement[1] + 1) % E.R])[None]
    assert ver.verify(inst2, out, frw.ENC_CANONICAL).tolist() == [0]
