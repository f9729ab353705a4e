"""The host half of the run-time-field interface, no device: frw_field_info through ctypes against Python integers, its refusals, and
frw_expand_field_host on compact records re-laid out from an oracle witness (tests/frw_testlib.compact_from_witness) -- every element
the oracle's integer times 2^256 mod BN254's Fr, a rejected record all zeros."""
import ctypes as C

import numpy as np
import pytest

import falcon_r1cs_amd as frw
from falcon_r1cs_amd import _lib

import field_cases as F
import frw_testlib as T

E_INVALID = -1


def _mod(p):
    return (C.c_uint64 * 4)(*F.limbs4(p))


@pytest.mark.parametrize("name", list(F.MODULI))
def test_field_info_equals_python(name):
    p, want = F.MODULI[name], F.consts(F.MODULI[name])
    info = frw.field_info(p)
    assert (info.modulus, info.one, info.r2, info.ninv32, info.bits) == (p, want["one"], want["r2"], want["ninv32"], want["bits"])
    s = _lib.FieldInfoStruct()
    assert frw.load_library().frw_field_info(_mod(p), C.byref(s)) == 0
    assert list(s.one) == F.limbs4(want["one"]) and list(s.modulus) == F.limbs4(p)


def test_field_info_bn254_one_is_the_published_constant():
    s = _lib.FieldInfoStruct()
    assert frw.load_library().frw_field_info(_mod(F.BN254), C.byref(s)) == 0
    assert tuple(s.one) == F.BN254_ONE_LIMBS


def test_refusals_and_null_pointers():
    lib = frw.load_library()
    s = _lib.FieldInfoStruct()
    for name, p in F.REFUSED.items():
        assert lib.frw_field_info(_mod(p), C.byref(s)) == E_INVALID, name
        with pytest.raises(frw.FrwError):
            frw.field_info(p)
    assert lib.frw_field_info(None, C.byref(s)) == E_INVALID
    assert lib.frw_field_info(_mod(F.BN254), None) == E_INVALID
    enc = C.c_int(-7)
    assert lib.frw_ctx_field_encoding(None, _mod(F.BN254), C.byref(enc)) == E_INVALID and enc.value == -7
    assert lib.frw_expand_field_dev(None, 9, 1, None, frw.ENC_FIELD_BASE, None, None, None) == E_INVALID
    buf = np.zeros(16, dtype=np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.frw_expand_field_host(None, 9, 1, p, p, p) == E_INVALID
    assert lib.frw_expand_field_host(_mod(F.BN254), 9, 1, None, p, p) == E_INVALID
    assert lib.frw_expand_field_host(_mod(F.BN254), 9, 1, p, None, p) == E_INVALID
    assert lib.frw_expand_field_host(_mod(F.BN254), 9, 1, p, p, None) == E_INVALID
    assert lib.frw_expand_field_host(_mod(F.BN254), 8, 1, p, p, p) == E_INVALID
    assert lib.frw_expand_field_host(_mod(F.BN254 - 1), 9, 0, None, None, None) == E_INVALID
    assert lib.frw_expand_field_host(_mod(F.BN254), 9, 0, None, None, None) == 0


def test_expand_field_host_on_an_oracle_witness(oracle):
    logn = 9
    lib = frw.load_library()
    L, CL = frw.layout(logn), frw.compact_layout(logn)
    sig, pk, hm = frw.synth_triples(logn, 1, seed=254)
    wit, inst, st = oracle.witness_ntt_verify(logn, sig, pk, hm, 1)
    cwit, cinst, _ = oracle.witness_ntt_verify(logn, sig, pk, hm, 0)                   # the integers themselves
    assert st.tolist() == [0]
    good = np.frombuffer(T.compact_from_witness(logn, wit[0], inst[0], CL), dtype=np.uint8)
    rejected = np.zeros(CL.bytes_per_signature, dtype=np.uint8)                        # what the producer leaves for a refused signature
    rejected[CL.status_off:CL.status_off + 4] = np.array([frw.ST_COEFF_RANGE], dtype=np.uint32).view(np.uint8)
    comp = np.stack([good, rejected, good])
    w2 = np.full((3, L.num_witness, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    i2 = np.full((3, L.num_instance, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for p in (F.BN254, F.BLS12_381):
        assert lib.frw_expand_field_host(_mod(p), logn, 3, ptr(comp), ptr(w2), ptr(i2)) == 0
        want_w = [F.mont(x, p) for x in T.limbs_to_ints(cwit[0])]
        want_i = [F.mont(x, p) for x in T.limbs_to_ints(cinst[0])]
        for k in (0, 2):
            assert T.limbs_to_ints(w2[k]) == want_w and T.limbs_to_ints(i2[k]) == want_i
        assert not w2[1].any() and not i2[1].any()
    # BLS12-381's own modulus: the bytes of frw_expand_host
    w3, i3 = np.empty_like(w2), np.empty_like(i2)
    assert lib.frw_expand_host(logn, 3, ptr(comp), ptr(w3), ptr(i3)) == 0
    assert np.array_equal(w2, w3) and np.array_equal(i2, i3)
    # and the Python face
    w4, _ = frw.expand_field_host(F.BN254, logn, comp[:1])
    assert T.limbs_to_ints(w4[0]) == [F.mont(x, F.BN254) for x in T.limbs_to_ints(cwit[0])]
