"""A constraint system over a run-time modulus, where no GPU is needed (include/frw.h frw_r1cs_export_field, frw_r1csf_*;
falcon-r1cs_amd/csrc/frw_r1cs_field.h).

* frw_r1cs_export_field against the ORACLE run over that modulus -- oracle/ark_sim.ConstraintSystem(p), the restated circuit,
  to_matrices() -- entry by entry, with the comparison of tests/test_r1cs_export.py: the product lifts the host mirror's BLS12-381
  matrices, the oracle builds the circuit over p from the gadget definitions, and neither knows of the other.
* the refusals, on device -1 (which no machine has, so validation is seen to come first with a GPU and without).
* the stand-alone program tests/cpp/test_r1cs_field_host.cpp under -fsanitize=address,undefined: the arithmetic, the lift, the
  2^200 guard on a doctored matrix, the parser.  Nothing sanitized is loaded into Python."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import falcon_r1cs_amd as frw
import field_cases as F
import frw_testlib as T
from oracle import falcon_gadgets as G
from oracle.ark_sim import ConstraintSystem
from test_r1cs_export import read_r1cs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CIRCUITS = {0: G.FalconNTTVerificationCircuit, 1: G.FalconDualNTTVerificationCircuit, 2: G.FalconSchoolBookVerificationCircuit}
INVALID_ARG, NO_DEVICE = -1, -2


def limbs(p):
    return (C.c_uint64 * 4)(*F.limbs4(p))


def assert_export_equals_oracle(tmp_path, circuit, name):
    logn, p = 9, F.MODULI[name]
    sig, pk, hm, _ = T.random_triple(logn, random.Random(13))
    cs = ConstraintSystem(p)
    CIRCUITS[circuit](sig.tolist(), pk.tolist(), hm.tolist(), logn).generate_constraints(cs, True)
    assert cs.is_satisfied()
    want = cs.to_matrices()
    path = tmp_path / "c.r1cs"
    cnt = frw.r1cs_export_field(circuit, logn, p, path)
    ni, nw, nc, mats = read_r1cs(path)
    assert (ni, nw, nc) == (cs.num_instance_variables(), cs.num_witness_variables(), cs.num_constraints()) == tuple(cnt[:3])
    assert cnt[3:] == [len(m[1]) for m in mats]
    for (ptr, col, val), rows in zip(mats, want):
        assert int(ptr[-1]) == sum(len(r) for r in rows)
        flat_cols = np.fromiter((c for r in rows for c, _ in r), dtype=np.uint32)
        assert np.array_equal(col, flat_cols)
        assert np.array_equal(np.diff(ptr.astype(np.int64)), np.fromiter((len(r) for r in rows), dtype=np.int64))
        flat_vals = b"".join(v.to_bytes(32, "little") for r in rows for _, v in r)
        assert val.tobytes() == flat_vals


@pytest.mark.parametrize("name", ["bn254", "2^160+7"])
@pytest.mark.parametrize("circuit", [0, 1])
def test_exported_matrices_over_p_equal_the_oracle_run_over_p(tmp_path, circuit, name):
    assert_export_equals_oracle(tmp_path, circuit, name)


def test_schoolbook_matrices_over_bn254_equal_the_oracle_run_over_p(tmp_path):
    assert_export_equals_oracle(tmp_path, 2, "bn254")


def test_the_group_order_itself_gives_the_export_back(tmp_path):
    """BLS12-381's own modulus is admissible, and the lift reduced mod r is the residue it came from: byte for byte frw_r1cs_export."""
    lib = frw.load_library()
    a, b = tmp_path / "r.r1cs", tmp_path / "lifted.r1cs"
    assert lib.frw_r1cs_export(0, 9, str(a).encode(), None) == 0
    frw.r1cs_export_field(0, 9, F.BLS12_381, b)
    assert a.read_bytes() == b.read_bytes()


def cubic(top):
    """x^3 + x + 5 = y (examples/custom_r1cs.py) with the 5 replaced by `top`: counts and the three pointer arrays, plus what they point into"""
    ONE, Y, X, X2, X3 = range(5)
    rows = ([[(1, X)], [(1, X2)], [(1, X3), (1, X), (top, ONE)]], [[(1, X)], [(1, X)], [(1, ONE)]], [[(1, X2)], [(1, X3)], [(1, Y)]])
    ptr = [np.array([0] + list(np.cumsum([len(r) for r in m])), dtype=np.uint64) for m in rows]
    col = [np.array([c for r in m for _, c in r], dtype=np.uint32) for m in rows]
    val = [np.array([F.limbs4(v) for r in m for v, _ in r], dtype=np.uint64) for m in rows]
    return ptr, col, val


def load_csr(p, ptr, col, val, counts=None):
    lib = frw.load_library()
    counts = (C.c_uint64 * 6)(*(counts or (2, 3, len(ptr[0]) - 1, len(col[0]), len(col[1]), len(col[2]))))
    three = [(C.c_void_p * 3)(*[a.ctypes.data_as(C.c_void_p) if a is not None else None for a in arrs]) for arrs in (ptr, col, val)]
    h = C.c_void_p(1)
    rc = lib.frw_r1csf_load_csr(-1, limbs(p), counts, *three, C.byref(h))
    assert not h.value
    return rc, lib.frw_last_error().decode()


@pytest.mark.parametrize("name", sorted(F.REFUSED))
def test_an_inadmissible_modulus_is_refused_everywhere(tmp_path, name):
    lib = frw.load_library()
    p = F.REFUSED[name]
    h = C.c_void_p()
    assert lib.frw_r1cs_export_field(0, 9, limbs(p), str(tmp_path / "x.r1cs").encode(), None) == INVALID_ARG
    assert "modulus" in lib.frw_last_error().decode()
    assert not (tmp_path / "x.r1cs").exists()
    assert lib.frw_r1csf_load(-1, 0, 9, limbs(p), C.byref(h)) == INVALID_ARG and not h.value
    assert load_csr(p, *cubic(5))[0] == INVALID_ARG
    assert lib.frw_r1csf_load_file(-1, limbs(p), str(tmp_path / "x.r1cs").encode(), C.byref(h)) == INVALID_ARG and not h.value


def test_validation_comes_first_then_the_device(tmp_path):
    lib = frw.load_library()
    p = F.BN254
    # well formed, the largest value there is: only the device is missing
    assert load_csr(p, *cubic(p - 1))[0] == NO_DEVICE
    h = C.c_void_p()
    assert lib.frw_r1csf_load(-1, 0, 9, limbs(p), C.byref(h)) == NO_DEVICE and not h.value
    # a value >= p -- below BLS12-381's group order, which frw_r1cs_load_csr would take
    rc, why = load_csr(p, *cubic(p))
    assert rc == INVALID_ARG and "matrix A, row 2" in why and "modulus" in why
    # the framing errors frw_r1cs_load_csr lists
    ptr, col, val = cubic(5)
    col[1][1] = 5
    rc, why = load_csr(p, ptr, col, val)
    assert rc == INVALID_ARG and "matrix B, row 1" in why
    ptr, col, val = cubic(5)
    ptr[2][1], ptr[2][2] = 2, 1
    rc, why = load_csr(p, ptr, col, val)
    assert rc == INVALID_ARG and "matrix C, row 1" in why
    ptr, col, val = cubic(5)
    ptr[0][0] = 1
    assert load_csr(p, ptr, col, val)[0] == INVALID_ARG
    ptr, col, val = cubic(5)
    ptr[0][3] = 4
    assert load_csr(p, ptr, col, val)[0] == INVALID_ARG
    ptr, col, val = cubic(5)
    assert load_csr(p, ptr, col, val, counts=(0, 3, 3, 5, 3, 3))[0] == INVALID_ARG           # no instance variable
    assert load_csr(p, ptr, col, val, counts=(2, (1 << 30) - 2, 3, 5, 3, 3))[0] == INVALID_ARG   # 2^30 variables
    assert load_csr(p, ptr, col, [val[0], None, val[2]])[0] == INVALID_ARG
    # files: the export over p loads as far as the device; cut short, another magic, absent
    good = tmp_path / "ntt9.r1cs"
    frw.r1cs_export_field(0, 9, p, good)
    raw = good.read_bytes()
    assert lib.frw_r1csf_load_file(-1, limbs(p), str(good).encode(), C.byref(h)) == NO_DEVICE
    # ... and the same file is refused over a modulus its values do not fit
    assert lib.frw_r1csf_load_file(-1, limbs(F.LOW), str(good).encode(), C.byref(h)) == INVALID_ARG
    assert "modulus" in lib.frw_last_error().decode()
    for name, data in (("short", raw[:-1]), ("long", raw + b"\0"), ("magic", b"FRWR1CS2" + raw[8:])):
        bad = tmp_path / (name + ".r1cs")
        bad.write_bytes(data)
        assert lib.frw_r1csf_load_file(-1, limbs(p), str(bad).encode(), C.byref(h)) == INVALID_ARG, name
    assert lib.frw_r1csf_load_file(-1, limbs(p), str(tmp_path / "absent.r1cs").encode(), C.byref(h)) == INVALID_ARG
    # arguments
    assert lib.frw_r1csf_load(-1, 3, 9, limbs(p), C.byref(h)) == INVALID_ARG
    assert lib.frw_r1csf_load(-1, 0, 8, limbs(p), C.byref(h)) == INVALID_ARG
    assert lib.frw_r1csf_load(-1, 0, 9, limbs(p), None) == INVALID_ARG
    assert lib.frw_r1cs_export_field(0, 9, limbs(p), None, None) == INVALID_ARG


def test_a_null_handle_and_an_empty_batch():
    lib = frw.load_library()
    lib.frw_r1csf_free(None)
    assert lib.frw_r1csf_info(None, None) == INVALID_ARG
    assert lib.frw_r1csf_scratch_bytes(None, 7, 0) == 0
    assert lib.frw_r1csf_check_dev(None, 0, None, None, None, None, None, None, 0, None) == 0        # batch = 0 returns first
    assert lib.frw_r1csf_check_dev(None, 1, None, None, None, None, None, None, 0, None) == INVALID_ARG
    with pytest.raises(frw.FrwError):
        frw.r1cs_export_field(0, 9, 1 << 256, "/nonexistent/x.r1cs")


def test_the_host_side_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "r1cs_field_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(HERE, "cpp", "hip_host"),
                           "-I", os.path.join(ROOT, "falcon-r1cs_amd", "csrc"), "-o", exe, os.path.join(HERE, "cpp", "test_r1cs_field_host.cpp")])
    work = tmp_path / "files"
    work.mkdir()
    res = subprocess.run([exe, str(work)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert res.returncode == 0, res.stdout
    assert res.stdout.strip().endswith("r1cs_field_host: clean"), res.stdout
    assert " 0 failed" in res.stdout, res.stdout
