"""The field side of the QAP witness map over a run-time modulus, where no GPU is needed (include/frw.h frw_fft_field_info,
frw_qapf_domain; falcon-r1cs_amd/csrc/frw_qap_field.h).

* the test helper tests/qap_field_reference.py at p = BLS12-381's r, g = 7 against the oracle's oracle/qap.py on random systems
* frw_fft_field_info and frw_qapf_domain against Python integers over seven moduli, BN254's published 2^28-th root and ark-bls12-381's
  Montgomery limbs among them; the refusals
* the stand-alone program tests/cpp/test_qap_field_host.cpp under -fsanitize=address,undefined.  Nothing sanitized is loaded into Python."""
import ctypes as C
import os
import random
import subprocess

import pytest

import falcon_r1cs_amd as frw
import field_cases as F
import qap_field_reference as R
from oracle import qap

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INVALID_ARG = -1
CASES = [("bn254", 5, 28), ("bls12_377", 22, 47), ("pallas", 5, 32), ("bls12_381", 7, 32), ("ed25519_l", 2, 2), ("2^255-19", 2, 2),
         ("2^160+7", 5, 1)]
BN254_ROOT = 19103219067921713944291392827692070036145651957329286315305642004821462161904       # the published 2^28-th root of unity


def limbs(x):
    return (C.c_uint64 * 4)(*F.limbs4(x))


def test_the_helper_equals_the_oracle_over_bls12_381():
    rng = random.Random(7)
    p = qap.P
    for nc in (3, 4, 5, 6, 7, 13, 14, 15, 31, 40):
        for satisfied in (True, False):
            ni = rng.randrange(1, 4)
            az, bz = ([rng.randrange(p) for _ in range(nc)] for _ in range(2))
            cz = [a * b % p for a, b in zip(az, bz)]
            if not satisfied:
                cz[rng.randrange(nc)] += 1
            inputs = [1] + [rng.randrange(p) for _ in range(ni - 1)]
            want = qap.witness_map_from_products(az, bz, cz, ni, inputs)
            got = R.witness_map(p, 7, az, bz, cz, inputs)
            assert got == want
            tau = rng.randrange(2, p)
            assert R.check_identity(p, 7, az, bz, cz, inputs, got, tau) == qap.check_identity(az, bz, cz, ni, inputs, want, tau)
            lhs, rhs = R.check_identity(p, 7, az, bz, cz, inputs, got, tau)
            assert (lhs == rhs) == satisfied


@pytest.mark.parametrize("name,g,s", CASES)
def test_fft_field_info_against_python(name, g, s):
    p = F.MODULI[name]
    info = frw.fft_field_info(p, g)
    t = (p - 1) >> s
    assert (p - 1) == t << s and t & 1
    root = pow(g, t, p)
    assert (info.modulus, info.generator, info.two_adicity, info.two_adic_root) == (p, g, s, root)
    assert info.two_adic_root_mont == F.mont(root, p)
    assert pow(root, 1 << s, p) == 1 and pow(root, 1 << (s - 1), p) == p - 1
    assert R.two_adic_root(p, g) == (s, root)


def test_the_published_roots():
    assert frw.fft_field_info(F.BN254, 5).two_adic_root == BN254_ROOT == pow(5, (F.BN254 - 1) >> 28, F.BN254)
    qap.check_constants()
    got = frw.fft_field_info(F.BLS12_381, 7).two_adic_root_mont
    assert F.limbs4(got) == [0xB9B58D8C5F0E466A, 0x5B1B4C801819D7EC, 0x0AF53AE352A31E64, 0x5BF3ADDA19E9B27B]


def refused(fn, *args):
    with pytest.raises(frw.FrwError) as err:
        fn(*args)
    assert err.value.code == INVALID_ARG
    return str(err.value)


def test_fft_field_info_refusals():
    for g in (2, 3, 4, 9):                                                     # squares mod bn254's r
        assert pow(g, (F.BN254 - 1) // 2, F.BN254) == 1
        assert "square" in refused(frw.fft_field_info, F.BN254, g)
    assert pow(3, (F.ED25519_L - 1) // 2, F.ED25519_L) == 1
    assert "square" in refused(frw.fft_field_info, F.ED25519_L, 3)
    for name in ("bn254", "2^160+7"):
        p = F.MODULI[name]
        for g in (0, p, p + 1):
            assert "generator" in refused(frw.fft_field_info, p, g)
    for name in sorted(F.REFUSED):
        assert "modulus" in refused(frw.fft_field_info, F.REFUSED[name], 5)
        assert "modulus" in refused(frw.qapf_domain, F.REFUSED[name], 5, 3, 2)
    composite = (1 << 200) + 1                                                 # admissible to frw_field_info, and no prime: 257 divides it
    assert composite % 257 == 0 and frw.field_info(composite).bits == 201
    assert "prime" in refused(frw.fft_field_info, composite, 3)
    lib = frw.load_library()
    from falcon_r1cs_amd._lib import FftFieldInfoStruct
    out = FftFieldInfoStruct()
    assert lib.frw_fft_field_info(None, limbs(5), C.byref(out)) == INVALID_ARG
    assert lib.frw_fft_field_info(limbs(F.BN254), None, C.byref(out)) == INVALID_ARG
    assert lib.frw_fft_field_info(limbs(F.BN254), limbs(5), None) == INVALID_ARG
    assert lib.frw_qapf_domain(limbs(F.BN254), limbs(5), 3, 2, None) == INVALID_ARG


@pytest.mark.parametrize("coeffs", [1, 2, 3, 4, 5, (1 << 12) - 1, 1 << 12, (1 << 12) + 1, (1 << 22) - 1, 1 << 22])
def test_qapf_domain_against_python(coeffs):
    p, g = F.BN254, 5
    ni = 1 if coeffs < 3 else 2
    d = frw.qapf_domain(p, g, coeffs - ni, ni)
    want = R.Domain(p, g, coeffs)
    assert (d.log_size, d.size) == (want.log_size, want.size) and want.size >= coeffs > want.size // 2
    assert (d.group_gen, d.group_gen_inv, d.size_inv, d.generator_inv, d.vanishing_inv) == (
        want.group_gen, want.group_gen_inv, want.size_inv, want.generator_inv, want.vanishing_inv)
    assert pow(d.group_gen, d.size, p) == 1 and (d.size == 1 or pow(d.group_gen, d.size // 2, p) == p - 1)
    assert d.vanishing_inv * (pow(g, d.size, p) - 1) % p == 1


def test_qapf_domain_refusals():
    assert "2^22" in refused(frw.qapf_domain, F.BN254, 5, (1 << 22) - 1, 2)                       # 2^22 + 1 coefficients
    assert "PolynomialDegreeTooLarge" in refused(frw.qapf_domain, F.ED25519_L, 2, 3, 2)            # 2^3 > 2^2
    assert frw.qapf_domain(F.ED25519_L, 2, 2, 2).log_size == 2
    assert "PolynomialDegreeTooLarge" in refused(frw.qapf_domain, F.LOW, 5, 1, 2)                  # C + I = 3 where s = 1
    assert frw.qapf_domain(F.LOW, 5, 1, 1).log_size == 1
    assert "coset" in refused(frw.qapf_domain, F.LOW, F.LOW - 1, 1, 1)                             # g^n = 1
    assert "PolynomialDegreeTooLarge" in refused(frw.qapf_domain, F.BN254, 5, 1 << 40, 2)


def test_a_null_handle_and_an_empty_batch():
    lib = frw.load_library()
    lib.frw_qapf_free(None)
    assert lib.frw_qapf_info(None, None) == INVALID_ARG
    out = C.c_void_p(1)
    assert lib.frw_qapf_create(None, limbs(5), C.byref(out)) == INVALID_ARG and not out.value
    assert lib.frw_qapf_witness_map_dev(None, 0, None, None, None, None, None, 0, None) == 0         # batch = 0 returns first
    assert lib.frw_qapf_witness_map_dev(None, 1, None, None, None, None, None, 0, None) == INVALID_ARG


def test_the_host_side_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "qap_field_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(HERE, "cpp", "hip_host"),
                           "-I", os.path.join(ROOT, "falcon-r1cs_amd", "csrc"), "-o", exe, os.path.join(HERE, "cpp", "test_qap_field_host.cpp")])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert res.returncode == 0, res.stdout
    assert res.stdout.strip().endswith("qap_field_host: clean"), res.stdout
    assert " 0 failed" in res.stdout, res.stdout
