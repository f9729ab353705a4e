"""The device verifier's C ABI where no GPU is needed (frw_groth16_vk_load_dev, frw_groth16_prepare_inputs_dev, frw_groth16_verify_dev,
frw_groth16_verify_workspace_bytes): refusals, not results -- no device means an error and never a host fallback, and a key loaded on the
host has no device part to prepare inputs with."""
import ctypes as C
import random

import numpy as np
import pytest

import falcon_r1cs_amd as frw
from oracle import bls12_381 as E


def _vk_limbs(num_public, seed=5):
    rng = random.Random(seed)
    pts = [E.mul(E.G1, rng.randrange(1, E.R)) for _ in range(num_public + 1)]
    g2 = [E.g2_to_limbs(E.g2_mul(E.G2, rng.randrange(1, E.R))) for _ in range(3)]
    flat = E.to_limbs(E.mul(E.G1, rng.randrange(1, E.R))) + g2[0] + g2[1] + g2[2]
    for p in pts:
        flat += E.to_limbs(p)
    return np.array(flat, dtype=np.uint64)


def test_device_load_without_a_device_is_an_error_not_a_fallback():
    lib = frw.load_library()
    if lib.frw_device_count() > 0:
        pytest.skip("a GPU is present; the refusal path is exercised on the CPU box")
    vk = _vk_limbs(2)
    h = C.c_void_p()
    assert lib.frw_groth16_vk_load_dev(0, vk.ctypes.data_as(C.c_void_p), 3, 0, C.byref(h)) == -2          # FRW_E_NO_DEVICE
    assert not h.value
    with pytest.raises(frw.FrwError) as ei:
        frw.Groth16Verifier(vk, device=0)
    assert ei.value.code == -2


def test_device_load_refuses_vouching_and_null_pointers():
    lib = frw.load_library()
    vk = _vk_limbs(2)
    h = C.c_void_p(1234)
    # FRW_VK_POINTS_ARE_CHECKED: checking every point is what the device load is for; it is refused whatever the device
    assert lib.frw_groth16_vk_load_dev(0, vk.ctypes.data_as(C.c_void_p), 3, frw.VK_POINTS_ARE_CHECKED, C.byref(h)) == -1
    assert not h.value
    assert lib.frw_groth16_vk_load_dev(0, None, 3, 0, C.byref(h)) == -1
    assert lib.frw_groth16_vk_load_dev(0, vk.ctypes.data_as(C.c_void_p), 0, 0, C.byref(h)) == -1
    assert lib.frw_groth16_vk_load_dev(0, vk.ctypes.data_as(C.c_void_p), 3, 0, None) == -1


def test_a_host_key_has_no_device_part():
    lib = frw.load_library()
    ver = frw.Groth16Verifier(_vk_limbs(2))
    h = ver._h
    assert lib.frw_groth16_verify_workspace_bytes(h, 1) == 0
    assert lib.frw_groth16_verify_workspace_bytes(None, 1) == 0
    buf = (C.c_uint64 * 64)()
    acc = (C.c_int32 * 1)()
    p = C.cast(buf, C.c_void_p)
    # a host-loaded key, then a null key: FRW_E_INVALID_ARG before any device is touched
    for key in (h, None):
        assert lib.frw_groth16_prepare_inputs_dev(key, 1, p, frw.ENC_MONTGOMERY, p, p, p, 4096, None) == -1
        assert lib.frw_groth16_verify_dev(key, 1, p, frw.ENC_MONTGOMERY, p, 0, C.cast(acc, C.c_void_p), p, 4096, None) == -1
    # and the host path of the same key is what it was
    assert ver.verify(np.zeros((1, 3, 4), dtype=np.uint64), np.zeros((1, 48), dtype=np.uint64)).tolist() == [-1]
    ver.close()
