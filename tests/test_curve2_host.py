"""The curve side of the multi-scalar multiplication over a run-time Fq2, where no GPU is needed (include/frw.h frw_curve2_info,
frw_curve2_check_points, frw_curve2_scalar_mul; falcon-r1cs_amd/csrc/frw_curve2.h).

* the two curves of tests/curve2_reference.py: BN254's G2 with its derived generator (r G is the point at infinity) and the curve over
  Pallas' Fq2 with beta = 5; the shortcut the GPU tests take for their expected sums -- one multiple of G -- against direct double-and-add
  at n = 64
* the three host calls against Python integers over both curves; every refusal
* the stand-alone program tests/cpp/test_curve2_host.cpp under -fsanitize=address,undefined.  Nothing sanitized is loaded into Python."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import falcon_r1cs_amd as frw
import curve2_reference as R
import field_cases as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INVALID_ARG = -1
NAMES = sorted(R.CURVES)


def desc(c):
    return (c.q, c.r, c.beta, c.b)


def test_the_reference_curves():
    g2 = R.BN254_G2
    assert g2.beta == g2.q - 1 and R.f2_mul(g2, g2.b, (9, 1)) == (3, 0)
    assert R.on_curve(g2, g2.g) and g2.g is not None
    assert R.mul(g2, g2.r, g2.g) is None and R.mul(g2, g2.r + 1, g2.g) == g2.g
    ext = R.PALLAS_EXT
    assert ext.beta == 5 and ext.order is None and R.on_curve(ext, ext.g)
    for c in (g2, ext):
        assert R.add(c, c.g, R.neg(c, c.g)) is None
        two = R.add(c, c.g, c.g)
        assert R.on_curve(c, two) and R.mul(c, 2, c.g) == two and R.add(c, two, R.neg(c, c.g)) == c.g


@pytest.mark.parametrize("name", NAMES)
def test_the_progression_shortcut_equals_double_and_add(name):
    c = R.CURVES[name]
    rng = random.Random(11)
    pts = R.progression(c, 64, 12345, 678)
    ks = [rng.randrange(c.r) for _ in pts]
    want = None
    for k, p in zip(ks, pts):
        want = R.add(c, want, R.mul(c, k, p))
    assert R.progression_sum(c, ks, 12345, 678) == want


@pytest.mark.parametrize("name", NAMES)
def test_curve2_info_against_python(name):
    c = R.CURVES[name]
    info = frw.curve2_info(*desc(c))
    assert (info.base_bits, info.scalar_bits) == (c.q.bit_length(), c.r.bit_length())
    assert info.b_mont == (F.mont(c.b[0], c.q), F.mont(c.b[1], c.q))
    assert info.one_mont == F.mont(1, c.q)
    assert info.nonresidue_mont == F.mont(c.beta, c.q)
    assert info.scalar_one_mont == F.mont(1, c.r)
    assert info.nonresidue_is_minus_one == (c.beta == c.q - 1)


@pytest.mark.parametrize("name", NAMES)
def test_scalar_mul_against_python(name):
    c = R.CURVES[name]
    rng = random.Random(5)
    p = R.mul(c, rng.randrange(1, c.r), c.g)
    ks = [0, 1, 2, c.r - 1, c.r, c.r + 1, (1 << 256) - 1] + [rng.randrange(1 << 256) for _ in range(3)]
    got = R.unpack(c, frw.curve2_scalar_mul(*desc(c), R.pack(c, [p] * len(ks)), R.scalars(ks)))
    assert got == [R.mul(c, k, p) for k in ks]
    assert got[0] is None and got[1] == p
    if c.order:
        assert got[3] == R.neg(c, p) and got[4] is None and got[5] == p
    # the point at infinity as input
    assert R.unpack(c, frw.curve2_scalar_mul(*desc(c), R.pack(c, [None, None]), R.scalars([0, 12345]))) == [None, None]
    assert frw.curve2_scalar_mul(*desc(c), np.zeros((0, 16), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64)).shape == (0, 16)


@pytest.mark.parametrize("name", NAMES)
def test_check_points_names_the_first_bad_one(name):
    c = R.CURVES[name]
    pts = R.progression(c, 6, 3, 5) + [None]
    good = R.pack(c, pts)
    assert frw.curve2_check_points(*desc(c), good) == -1
    assert frw.curve2_check_points(*desc(c), good[:0]) == -1
    off = good.copy()
    off[4, 12:] = F.limbs4(F.mont((pts[4][1][1] + 1) % c.q, c.q))          # y.c1 + 1: off the curve
    off[5, 0] ^= 1                                                        # a later bad one is not the one named
    assert frw.curve2_check_points(*desc(c), off) == 4
    for comp in range(4):                                                 # the same residue, not canonical, in every component
        big = good.copy()
        v = F.mont((pts[2][0] + pts[2][1])[comp], c.q)
        assert v + c.q < 1 << 256
        big[2, 4 * comp:4 * comp + 4] = F.limbs4(v + c.q)
        assert frw.curve2_check_points(*desc(c), big) == 2
    zero_x = good.copy()
    zero_x[0, :8] = 0                                                     # (0, y): only ALL zero is infinity
    assert frw.curve2_check_points(*desc(c), zero_x) == 0
    with pytest.raises(frw.FrwError) as e:
        frw.curve2_scalar_mul(*desc(c), off, R.scalars([1] * len(pts)))
    assert e.value.code == INVALID_ARG and "point 4" in str(e.value)


Q, RR = R.BN254_G2.q, R.BN254_G2.r
B = R.BN254_G2.b


@pytest.mark.parametrize("what,q,r,beta,b,word", [
    ("q even", Q - 1, RR, 5, B, "base modulus"), ("q = 2^160", 1 << 160, RR, 5, (3, 4), "base modulus"),
    ("q > 2^255", (1 << 255) + 1, RR, 5, B, "base modulus"), ("q = 0", 0, RR, 5, B, "base modulus"),
    ("r even", Q, RR - 1, Q - 1, B, "scalar modulus"), ("r = 2^160", Q, 1 << 160, Q - 1, B, "scalar modulus"),
    ("r > 2^255", Q, (1 << 255) + 1, Q - 1, B, "scalar modulus"),
    ("beta = 0", Q, RR, 0, B, "non-residue is zero"), ("beta = q", Q, RR, Q, B, "non-residue is not below"),
    ("beta > q", Q, RR, (1 << 256) - 1, B, "non-residue is not below"),
    ("b = 0", Q, RR, Q - 1, (0, 0), "b = 0"), ("b.c0 = q", Q, RR, Q - 1, (Q, 1), "component of b"),
    ("b.c1 = q", Q, RR, Q - 1, (1, Q), "component of b"), ("b.c1 > q", Q, RR, Q - 1, (0, (1 << 256) - 1), "component of b")])
def test_every_refusal_of_the_descriptor(what, q, r, beta, b, word):
    for call in (lambda: frw.curve2_info(q, r, beta, b), lambda: frw.curve2_check_points(q, r, beta, b, np.zeros((1, 16), dtype=np.uint64)),
                 lambda: frw.curve2_scalar_mul(q, r, beta, b, np.zeros((1, 16), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64))):
        with pytest.raises(frw.FrwError) as e:
            call()
        assert e.value.code == INVALID_ARG and word in str(e.value), (what, str(e.value))


def test_values_beyond_four_limbs_are_refused_in_their_own_name():
    for beta, b in ((1 << 256, B), (-1, B), (Q - 1, (1 << 256, 0)), (Q - 1, (0, -1))):
        with pytest.raises(frw.FrwError) as e:
            frw.curve2_info(Q, RR, beta, b)
        assert e.value.code == INVALID_ARG and "does not fit four limbs" in str(e.value)


def test_half_of_b_may_be_zero_and_any_beta_below_q_is_taken():
    assert frw.curve2_info(Q, RR, Q - 1, (0, 4)).b_mont == (0, F.mont(4, Q))
    assert frw.curve2_info(Q, RR, Q - 1, (3, 0)).b_mont == (F.mont(3, Q), 0)
    assert not frw.curve2_info(Q, RR, Q - 2, B).nonresidue_is_minus_one
    assert not frw.curve2_info(Q, RR, 1, B).nonresidue_is_minus_one          # (a residue: the caller's business)


def test_null_pointers_and_the_device_calls_without_a_handle():
    from falcon_r1cs_amd._lib import Curve2InfoStruct, Curve2Struct, Msmf2InfoStruct
    lib = frw.load_library()
    c = R.BN254_G2
    cs = Curve2Struct((C.c_uint64 * 4)(*F.limbs4(c.q)), (C.c_uint64 * 4)(*F.limbs4(c.r)), (C.c_uint64 * 4)(*F.limbs4(c.beta)),
                      (C.c_uint64 * 8)(*F.limbs4(c.b[0]), *F.limbs4(c.b[1])))
    info, bad = Curve2InfoStruct(), C.c_int64(7)
    assert lib.frw_curve2_info(C.byref(cs), C.byref(info)) == 0
    assert lib.frw_curve2_info(None, C.byref(info)) == INVALID_ARG
    assert lib.frw_curve2_info(C.byref(cs), None) == INVALID_ARG
    assert lib.frw_curve2_check_points(C.byref(cs), 1, None, C.byref(bad)) == INVALID_ARG
    assert lib.frw_curve2_check_points(C.byref(cs), 0, None, None) == INVALID_ARG
    assert lib.frw_curve2_scalar_mul(C.byref(cs), 1, None, None, None) == INVALID_ARG
    assert lib.frw_msmf2_info(None, C.byref(Msmf2InfoStruct())) == INVALID_ARG
    assert lib.frw_msmf2_workspace_bytes(None, 1) == 0
    assert lib.frw_msmf2_dev(None, 1, None, 0, 0, 0, None, None, 0, None) == INVALID_ARG
    h = C.c_void_p()
    pts = R.pack(c, [c.g])
    assert lib.frw_msmf2_load(0, None, 1, pts.ctypes.data_as(C.c_void_p), 0, C.byref(h)) == INVALID_ARG
    assert lib.frw_msmf2_load(0, C.byref(cs), 1, None, 0, C.byref(h)) == INVALID_ARG
    assert lib.frw_msmf2_load(0, C.byref(cs), 1, pts.ctypes.data_as(C.c_void_p), 0, None) == INVALID_ARG
    # refused before any device is looked at: the count and the descriptor
    assert lib.frw_msmf2_load(0, C.byref(cs), 0, pts.ctypes.data_as(C.c_void_p), 0, C.byref(h)) == INVALID_ARG
    assert lib.frw_msmf2_load(0, C.byref(cs), (1 << 22) + 1, pts.ctypes.data_as(C.c_void_p), 0, C.byref(h)) == INVALID_ARG
    assert b"2^22" in lib.frw_last_error()
    lib.frw_msmf2_free(None)


def test_the_host_side_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "curve2_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(HERE, "cpp", "hip_host"),
                           "-I", os.path.join(ROOT, "falcon-r1cs_amd", "csrc"), "-o", exe, os.path.join(HERE, "cpp", "test_curve2_host.cpp")])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert res.returncode == 0, res.stdout
    assert res.stdout.strip().endswith("curve2_host: clean"), res.stdout
    assert " 0 failed" in res.stdout, res.stdout
