"""Groth16 PROVING keys in ark-serialize's wire format, the part that needs no device: the four entry points exist and frw.h declares
them, frw_groth16_pk_wire_bytes is the format table's sum, frw_groth16_pk_wire_info walks the framing of keys that tests/pk_wire_ref.py
built (a second restatement of the format, in Python integers) and refuses every framing the rules exclude without reading past the
buffer, and the two device entry points answer FRW_E_NO_DEVICE / FRW_E_INVALID_ARG without a device."""
import ctypes as C
import os

import numpy as np
import pytest

import falcon_r1cs_amd as frw
import pk_wire_ref as P
from oracle import bls12_381 as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [True, False]
SYMBOLS = ["frw_groth16_pk_wire_bytes", "frw_groth16_pk_wire_info", "frw_groth16_pk_load_wire_dev", "frw_groth16_pk_to_wire_dev"]
INVALID, NO_DEVICE = -1, -2


def _multiples(count):
    """G1, 2 G1, ... and the same in G2 (one addition each: the framing does not care what the points are, but they are real ones)"""
    g1, g2, a, b = [], [], None, None
    for _ in range(count):
        a, b = E.add(a, E.G1), E.g2_add(b, E.G2)
        g1.append(a)
        g2.append(b)
    return g1, g2


_G1, _G2 = _multiples(40)


def small_key(num_instance=3, num_witness=5, domain_size=8):
    nv = num_instance + num_witness
    pick = lambda first, count: [None if (first + i) % 5 == 4 else _G1[(first + i) % 40] for i in range(count)]
    return {"vk": {"alpha_g1": _G1[0], "beta_g2": _G2[1], "gamma_g2": _G2[2], "delta_g2": _G2[3], "gamma_abc_g1": pick(7, num_instance)},
            "beta_g1": _G1[4], "delta_g1": _G1[5],
            "a_query": pick(0, nv), "b_g1_query": pick(11, nv), "b_g2_query": [None if i % 3 == 1 else _G2[(i + 6) % 40] for i in range(nv)],
            "h_query": pick(3, domain_size - 1), "l_query": pick(9, num_witness)}


def _info(data, compressed):
    lib = frw.load_library()
    from falcon_r1cs_amd._lib import Groth16PkWireInfoStruct
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(bytes(data) or b"\0")
    out = Groth16PkWireInfoStruct()
    return lib.frw_groth16_pk_wire_info(buf, len(data), 0 if compressed else 1, C.byref(out)), out


def test_the_four_symbols_exist_and_the_header_declares_them():
    lib = frw.load_library()
    header = open(os.path.join(ROOT, "include", "frw.h")).read()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None
        assert name + "(" in header
    assert "FRW_PK_POINTS_ARE_CHECKED" in header and "frw_groth16_pk_wire_info_t" in header


@pytest.mark.parametrize("compressed", MODES)
def test_wire_bytes_is_the_sum_of_the_format_table(compressed):
    lib = frw.load_library()
    mode = 0 if compressed else 1
    for ni, nw, n in [(1, 0, 2), (3, 5, 8), (3, 30, 64), (5, 124, 128), (2049, 1123456, 1 << 21)]:
        want = P.pk_bytes(ni, nw, n, compressed)
        assert lib.frw_groth16_pk_wire_bytes(ni, nw, n, mode) == want
        assert frw.groth16_pk_wire_bytes(ni, nw, n, compressed) == want
    assert lib.frw_groth16_pk_wire_bytes(3, 5, 8, 2) == 0 and lib.frw_groth16_pk_wire_bytes(3, 5, 8, -1) == 0
    assert lib.frw_groth16_pk_wire_bytes(0, 5, 8, mode) == 0           # no constant one
    assert lib.frw_groth16_pk_wire_bytes(3, 5, 96, mode) == 0          # not a power of two
    assert lib.frw_groth16_pk_wire_bytes(3, 5, 1, mode) == 0


@pytest.mark.parametrize("compressed", MODES)
@pytest.mark.parametrize("shape", [(1, 0, 2), (3, 5, 8), (4, 61, 64)])
def test_wire_info_returns_the_counts_and_offsets_the_helper_used(compressed, shape):
    key = small_key(*shape)
    data = P.pk_encode(key, compressed)
    assert len(data) == P.pk_bytes(*shape, compressed)
    rc, out = _info(data, compressed)
    assert rc == 0
    assert (out.num_instance, out.num_witness, out.domain_size) == shape
    offs = P.pk_offsets(key, compressed)
    assert {name: getattr(out, name + "_offset") for name in P.QUERIES} == offs
    got = frw.groth16_pk_wire_info(data, compressed)
    assert (got["num_instance"], got["num_witness"], got["domain_size"]) == shape and got["h_query_offset"] == offs["h_query"]
    # the other mode's framing does not fit these bytes
    assert _info(data, not compressed)[0] == INVALID


@pytest.mark.parametrize("compressed", MODES)
def test_wire_info_refuses_what_the_framing_rules_exclude(compressed):
    lib = frw.load_library()
    key = small_key()
    good = P.pk_encode(key, compressed)
    assert _info(good, compressed)[0] == 0
    assert _info(good[:-1], compressed)[0] == INVALID                                   # one byte short
    assert _info(good + b"\0", compressed)[0] == INVALID                                # one byte long
    assert _info(b"", compressed)[0] == INVALID and _info(good[:100], compressed)[0] == INVALID

    def variant(**changes):
        k = dict(key)
        k.update(changes)
        return P.pk_encode(k, compressed)
    assert _info(variant(b_g1_query=key["b_g1_query"] + [_G1[0]]), compressed)[0] == INVALID      # len(b_g1_query) != len(a_query)
    assert _info(variant(b_g2_query=key["b_g2_query"][:-1]), compressed)[0] == INVALID
    assert _info(variant(l_query=key["l_query"][:-1]), compressed)[0] == INVALID                  # len(l_query) + I != len(a_query)
    assert _info(variant(h_query=[_G1[i % 40] for i in range(95)]), compressed)[0] == INVALID     # len(h_query) + 1 = 96
    assert _info(variant(h_query=[]), compressed)[0] == INVALID                                   # n = 1
    no_instance = dict(key["vk"], gamma_abc_g1=[])
    assert _info(variant(vk=no_instance, l_query=key["a_query"]), compressed)[0] == INVALID       # I = 0 (everything else consistent)
    # a length field of 2^40 on a short buffer: the bytes END right after that field (and once inside it, once just before it); the
    # buffers are exactly that long, so a walker that trusted the field would read past them (tools/sanitize_cpu.sh shows such a read)
    head = P.pk_encode(dict(key, a_query=[], b_g1_query=[], b_g2_query=[], h_query=[], l_query=[]), compressed, {"a_query": 1 << 40})
    cut = head[:P.pk_offsets(key, compressed)["a_query"]]
    assert cut[-8:] == (1 << 40).to_bytes(8, "little")
    for short in (0, 1, 8):
        assert _info(cut[:len(cut) - short], compressed)[0] == INVALID
    assert _info(cut + good[len(cut):], compressed)[0] == INVALID                       # ... and with the key's own bytes behind it
    with pytest.raises(frw.FrwError) as ei:
        frw.groth16_pk_wire_info(good[:-1], compressed)
    assert ei.value.code == INVALID
    # null pointers and a bad mode
    buf = (C.c_uint8 * len(good)).from_buffer_copy(good)
    from falcon_r1cs_amd._lib import Groth16PkWireInfoStruct
    out = Groth16PkWireInfoStruct()
    assert lib.frw_groth16_pk_wire_info(None, len(good), 0, C.byref(out)) == INVALID
    assert lib.frw_groth16_pk_wire_info(buf, len(good), 0 if compressed else 1, None) == INVALID
    assert lib.frw_groth16_pk_wire_info(buf, len(good), 2, C.byref(out)) == INVALID


def test_dev_entry_points_without_a_device_and_with_bad_arguments():
    """a device index that no machine has: FRW_E_NO_DEVICE, never a host fallback; null pointers, a bad mode, unknown flags, a key in slices
    and bad framing: FRW_E_INVALID_ARG first"""
    from falcon_r1cs_amd._lib import Groth16KeyOpts
    lib = frw.load_library()
    nowhere = 1 << 20
    for compressed in MODES:
        mode = 0 if compressed else 1
        data = P.pk_encode(small_key(), compressed)
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        vk = np.zeros(84 + 12 * 3, dtype=np.uint64)
        vkp = vk.ctypes.data_as(C.c_void_p)
        load = lib.frw_groth16_pk_load_wire_dev
        for opts in (None, C.byref(Groth16KeyOpts(frw.KEY_TABLES, 0, 1)), C.byref(Groth16KeyOpts(frw.KEY_BARE, 0, 1))):
            for flags in (0, frw.PK_POINTS_ARE_CHECKED):
                h = C.c_void_p(5)
                assert load(nowhere, buf, len(data), mode, flags, opts, C.byref(h), vkp) == NO_DEVICE and not h.value
        h = C.c_void_p(5)
        assert load(nowhere, buf, len(data), mode, 0, None, C.byref(h), None) == NO_DEVICE and not h.value
        assert load(nowhere, buf, len(data), mode, 0, None, None, vkp) == INVALID
        for args in [(None, len(data), mode, 0, None), (buf, len(data), 2, 0, None), (buf, len(data), mode, 2, None),
                     (buf, len(data) - 1, mode, 0, None), (buf, len(data), 1 - mode, 0, None),
                     (buf, len(data), mode, 0, C.byref(Groth16KeyOpts(frw.KEY_BARE, 0, 2))),
                     (buf, len(data), mode, 0, C.byref(Groth16KeyOpts(frw.KEY_BARE, 1, 2))),
                     (buf, len(data), mode, 0, C.byref(Groth16KeyOpts(7, 0, 1)))]:
            h = C.c_void_p(5)
            assert load(nowhere, *args, C.byref(h), vkp) == INVALID and not h.value, args[1:4]
        # the export needs a key handle: a null one, null buffers and a bad mode are refused before any device is touched
        out = (C.c_uint8 * len(data))()
        assert lib.frw_groth16_pk_to_wire_dev(None, vkp, 3, mode, out, len(data)) == INVALID
    eng_less = frw.WitnessEngine.__new__(frw.WitnessEngine)            # (no device: only the library and an index nobody has)
    eng_less._lib, eng_less.device = lib, nowhere
    with pytest.raises(frw.FrwError) as ei:
        eng_less.groth16_pk_load_wire(P.pk_encode(small_key(), True))
    assert ei.value.code == NO_DEVICE
