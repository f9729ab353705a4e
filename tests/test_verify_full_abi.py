"""The full device verifier's C ABI where no GPU is needed (frw_groth16_verify_full_dev, frw_groth16_verify_full_workspace_bytes,
frw_diag_pairing_dev): the symbols exist, and the refusals -- no device is an error and never a host fallback, a key loaded on the host
has no device part, null pointers, unknown flags and a batched request without a seed are refused before any device is touched."""
import ctypes as C

import numpy as np
import pytest

import falcon_r1cs_amd as frw
from oracle import bls12_381 as E
from test_verify_dev_abi import _vk_limbs

NEW = ("frw_groth16_verify_full_dev", "frw_groth16_verify_full_workspace_bytes", "frw_diag_pairing_dev")


def test_the_new_symbols_are_exported():
    lib = C.CDLL(frw.lib_path())
    for name in NEW:
        assert hasattr(lib, name), name
    header = open(_header()).read()
    for name in NEW:
        assert name in header, name


def _header():
    import os
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frw.h")


def test_without_a_device_the_device_pairing_is_an_error_not_a_fallback():
    lib = frw.load_library()
    if lib.frw_device_count() > 0:
        pytest.skip("a GPU is present; the refusal path is exercised on the CPU box")
    g1 = np.array(E.to_limbs(E.G1), dtype=np.uint64)
    g2 = np.array(E.g2_to_limbs(E.G2), dtype=np.uint64)
    out = np.zeros(72, dtype=np.uint64)
    assert lib.frw_diag_pairing_dev(0, 1, g1.ctypes.data_as(C.c_void_p), g2.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == -2
    with pytest.raises(frw.FrwError) as ei:
        frw.diag_pairing_dev(g1, g2)
    assert ei.value.code == -2
    vk = _vk_limbs(2)
    h = C.c_void_p()
    assert lib.frw_groth16_vk_load_dev(0, vk.ctypes.data_as(C.c_void_p), 3, 0, C.byref(h)) == -2
    assert not h.value


def test_a_host_key_is_refused_and_has_no_workspace():
    lib = frw.load_library()
    ver = frw.Groth16Verifier(_vk_limbs(2))
    h = ver._h
    assert frw.VERIFY_BATCHED == 2
    for flags in (0, frw.VERIFY_POINTS_ARE_CHECKED, frw.VERIFY_BATCHED):
        assert lib.frw_groth16_verify_full_workspace_bytes(h, 1, flags) == 0
        assert lib.frw_groth16_verify_full_workspace_bytes(None, 1, flags) == 0
    assert ver.full_workspace_bytes(4) == 0
    buf = (C.c_uint64 * 64)()
    p = C.cast(buf, C.c_void_p)
    seed = (C.c_uint64 * 4)(1, 2, 3, 4)
    for key in (h, None):
        # a host-loaded key, then a null key: FRW_E_INVALID_ARG before any device is touched (batch = 0 included)
        for batch in (0, 1):
            assert lib.frw_groth16_verify_full_dev(key, batch, p, frw.ENC_MONTGOMERY, p, 0, None, p, None, p, 4096, None) == -1
        # null pointers, a bad encoding, an unknown flag, FRW_VERIFY_BATCHED without a seed (and with one: still no device part)
        assert lib.frw_groth16_verify_full_dev(key, 1, None, frw.ENC_MONTGOMERY, p, 0, None, p, None, p, 4096, None) == -1
        assert lib.frw_groth16_verify_full_dev(key, 1, p, 7, p, 0, None, p, None, p, 4096, None) == -1
        assert lib.frw_groth16_verify_full_dev(key, 1, p, frw.ENC_MONTGOMERY, p, 4, None, p, None, p, 4096, None) == -1
        assert lib.frw_groth16_verify_full_dev(key, 1, p, frw.ENC_MONTGOMERY, p, frw.VERIFY_BATCHED, None, p, p, p, 4096, None) == -1
        assert lib.frw_groth16_verify_full_dev(key, 1, p, frw.ENC_MONTGOMERY, p, frw.VERIFY_BATCHED, C.cast(seed, C.c_void_p), p, p, p, 4096,
                                               None) == -1
    ver.close()
