"""The curve side of the multi-scalar multiplication over a run-time curve, where no GPU is needed (include/frw.h frw_curve_info,
frw_curve_check_points, frw_curve_scalar_mul; falcon-r1cs_amd/csrc/frw_curve.h).

* the four curves of tests/curve_reference.py: the generator is on the curve and r G is the point at infinity; the shortcut the GPU tests
  take for their expected sums -- one multiple of G -- against direct double-and-add at n = 64
* the three host calls against Python integers over BN254 G1, Pallas, Vesta and Grumpkin; the refusals
* the stand-alone program tests/cpp/test_curve_host.cpp under -fsanitize=address,undefined.  Nothing sanitized is loaded into Python."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import falcon_r1cs_amd as frw
import curve_reference as R
import field_cases as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INVALID_ARG = -1
NAMES = sorted(R.CURVES)


@pytest.mark.parametrize("name", NAMES)
def test_the_reference_curves(name):
    c = R.CURVES[name]
    assert R.on_curve(c, c.g)
    assert R.mul(c, c.r, c.g) is None
    assert R.mul(c, c.r + 1, c.g) == c.g
    assert R.add(c, c.g, R.neg(c, c.g)) is None


def test_the_progression_shortcut_equals_double_and_add():
    c = R.BN254
    rng = random.Random(11)
    pts = R.progression(c, 64, 12345, 678)
    ks = [rng.randrange(c.r) for _ in pts]
    want = None
    for k, p in zip(ks, pts):
        want = R.add(c, want, R.mul(c, k, p))
    assert R.progression_sum(c, ks, 12345, 678) == want


@pytest.mark.parametrize("name", NAMES)
def test_curve_info_against_python(name):
    c = R.CURVES[name]
    info = frw.curve_info(c.q, c.r, c.b)
    assert (info.base_bits, info.scalar_bits) == (c.q.bit_length(), c.r.bit_length())
    assert info.b_mont == F.mont(c.b, c.q)
    assert info.one_mont == F.mont(1, c.q)
    assert info.scalar_one_mont == F.mont(1, c.r)


@pytest.mark.parametrize("name", NAMES)
def test_scalar_mul_against_python(name):
    c = R.CURVES[name]
    rng = random.Random(5)
    p = R.mul(c, rng.randrange(1, c.r), c.g)
    ks = [0, 1, 2, c.r - 1, c.r, c.r + 1, (1 << 256) - 1] + [rng.randrange(1 << 256) for _ in range(3)]
    got = R.unpack(c, frw.curve_scalar_mul(c.q, c.r, c.b, R.pack(c, [p] * len(ks)), R.scalars(ks)))
    assert got == [R.mul(c, k, p) for k in ks]
    assert got[0] is None and got[1] == p and got[3] == R.neg(c, p) and got[4] is None and got[5] == p
    # the point at infinity as input
    assert R.unpack(c, frw.curve_scalar_mul(c.q, c.r, c.b, R.pack(c, [None, None]), R.scalars([0, 12345]))) == [None, None]
    assert frw.curve_scalar_mul(c.q, c.r, c.b, np.zeros((0, 8), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64)).shape == (0, 8)


@pytest.mark.parametrize("name", NAMES)
def test_check_points_names_the_first_bad_one(name):
    c = R.CURVES[name]
    pts = R.progression(c, 6, 3, 5) + [None]
    good = R.pack(c, pts)
    assert frw.curve_check_points(c.q, c.r, c.b, good) == -1
    assert frw.curve_check_points(c.q, c.r, c.b, good[:0]) == -1
    off = good.copy()
    off[4, 4:] = F.limbs4(F.mont((pts[4][1] + 1) % c.q, c.q))              # y + 1: off the curve
    off[5, 0] ^= 1                                                        # a later bad one is not the one named
    assert frw.curve_check_points(c.q, c.r, c.b, off) == 4
    big = good.copy()
    x = F.mont(pts[2][0], c.q)
    assert x + c.q < 1 << 256
    big[2, :4] = F.limbs4(x + c.q)                                        # the same residue, not canonical
    assert frw.curve_check_points(c.q, c.r, c.b, big) == 2
    zero_x = good.copy()
    zero_x[0, :4] = 0                                                     # (0, y): only ALL zero is infinity
    assert frw.curve_check_points(c.q, c.r, c.b, zero_x) == 0
    with pytest.raises(frw.FrwError) as e:
        frw.curve_scalar_mul(c.q, c.r, c.b, off, R.scalars([1] * len(pts)))
    assert e.value.code == INVALID_ARG and "point 4" in str(e.value)


@pytest.mark.parametrize("what,q,r,b,word", [
    ("q even", R.BN254.q - 1, R.BN254.r, 3, "base modulus"), ("q = 2^160", 1 << 160, R.BN254.r, 3, "base modulus"),
    ("q > 2^255", (1 << 255) + 1, R.BN254.r, 3, "base modulus"), ("q = 0", 0, R.BN254.r, 3, "base modulus"),
    ("r even", R.BN254.q, R.BN254.r - 1, 3, "scalar modulus"), ("r = 2^160", R.BN254.q, 1 << 160, 3, "scalar modulus"),
    ("r > 2^255", R.BN254.q, (1 << 255) + 1, 3, "scalar modulus"), ("b = 0", R.BN254.q, R.BN254.r, 0, "b = 0"),
    ("b = q", R.BN254.q, R.BN254.r, R.BN254.q, "below"), ("b > q", R.BN254.q, R.BN254.r, (1 << 256) - 1, "below")])
def test_every_refusal_of_the_descriptor(what, q, r, b, word):
    for call in (lambda: frw.curve_info(q, r, b), lambda: frw.curve_check_points(q, r, b, np.zeros((1, 8), dtype=np.uint64)),
                 lambda: frw.curve_scalar_mul(q, r, b, np.zeros((1, 8), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64))):
        with pytest.raises(frw.FrwError) as e:
            call()
        assert e.value.code == INVALID_ARG and word in str(e.value), (what, str(e.value))


def test_a_b_beyond_four_limbs_is_refused_in_its_own_name():
    for b in (1 << 256, -1):
        with pytest.raises(frw.FrwError) as e:
            frw.curve_info(R.BN254.q, R.BN254.r, b)
        assert e.value.code == INVALID_ARG and "b does not fit four limbs" in str(e.value)


def test_null_pointers_and_the_device_calls_without_a_handle():
    from falcon_r1cs_amd._lib import CurveInfoStruct, CurveStruct, MsmfInfoStruct
    lib = frw.load_library()
    c = R.BN254
    cs = CurveStruct((C.c_uint64 * 4)(*F.limbs4(c.q)), (C.c_uint64 * 4)(*F.limbs4(c.r)), (C.c_uint64 * 4)(*F.limbs4(c.b)))
    info, bad = CurveInfoStruct(), C.c_int64(7)
    assert lib.frw_curve_info(None, C.byref(info)) == INVALID_ARG
    assert lib.frw_curve_info(C.byref(cs), None) == INVALID_ARG
    assert lib.frw_curve_check_points(C.byref(cs), 1, None, C.byref(bad)) == INVALID_ARG
    assert lib.frw_curve_check_points(C.byref(cs), 0, None, None) == INVALID_ARG
    assert lib.frw_curve_scalar_mul(C.byref(cs), 1, None, None, None) == INVALID_ARG
    assert lib.frw_msmf_info(None, C.byref(MsmfInfoStruct())) == INVALID_ARG
    assert lib.frw_msmf_workspace_bytes(None, 1) == 0
    assert lib.frw_msmf_dev(None, 1, None, 0, 0, 0, None, None, 0, None) == INVALID_ARG
    h = C.c_void_p()
    pts = R.pack(c, [c.g])
    assert lib.frw_msmf_load(0, None, 1, pts.ctypes.data_as(C.c_void_p), 0, C.byref(h)) == INVALID_ARG
    assert lib.frw_msmf_load(0, C.byref(cs), 1, None, 0, C.byref(h)) == INVALID_ARG
    assert lib.frw_msmf_load(0, C.byref(cs), 1, pts.ctypes.data_as(C.c_void_p), 0, None) == INVALID_ARG
    # refused before any device is looked at: the count and the descriptor
    assert lib.frw_msmf_load(0, C.byref(cs), 0, pts.ctypes.data_as(C.c_void_p), 0, C.byref(h)) == INVALID_ARG
    assert lib.frw_msmf_load(0, C.byref(cs), (1 << 22) + 1, pts.ctypes.data_as(C.c_void_p), 0, C.byref(h)) == INVALID_ARG
    assert b"2^22" in lib.frw_last_error()
    lib.frw_msmf_free(None)


def test_the_host_side_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "curve_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(HERE, "cpp", "hip_host"),
                           "-I", os.path.join(ROOT, "falcon-r1cs_amd", "csrc"), "-o", exe, os.path.join(HERE, "cpp", "test_curve_host.cpp")])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert res.returncode == 0, res.stdout
    assert res.stdout.strip().endswith("curve_host: clean"), res.stdout
    assert " 0 failed" in res.stdout, res.stdout
