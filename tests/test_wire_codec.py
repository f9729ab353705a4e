"""The wire codec on the host (frw_groth16_proofs_to_wire / _from_wire, frw_groth16_vk_to_wire / _vk_load_wire; frw_wire.h) against an
independent restatement of ark-serialize's format in Python integers (tests/wire_ref.py): bytes for bytes, limbs for limbs, every
malformed case refused alone in an otherwise valid batch -- and the refusals of the _dev entry points that need no device."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import falcon_r1cs_amd as frw
import wire_ref as W
from oracle import bls12_381 as E
from test_pairing_host import fr_limbs, make_statement, proof_limbs, vk_limbs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = E.Q
NEW = ["frw_groth16_proof_wire_bytes", "frw_groth16_vk_wire_bytes", "frw_groth16_proofs_to_wire", "frw_groth16_proofs_from_wire",
       "frw_groth16_proofs_to_wire_dev", "frw_groth16_proofs_from_wire_dev", "frw_groth16_verify_wire_workspace_bytes",
       "frw_groth16_verify_wire_dev", "frw_groth16_vk_to_wire", "frw_groth16_vk_load_wire", "frw_groth16_vk_load_wire_dev"]
MODES = [True, False]                                    # compressed?


def u64(v):
    return np.array(v, dtype=np.uint64).reshape(-1)


def g2neg(p):
    return None if p is None else (p[0], ((-p[1][0]) % Q, (-p[1][1]) % Q))


def points():
    """(G1 points, G2 points): k G, -k G for a spread of k, and infinity"""
    rng = random.Random(404)
    ks = [1, 2, 3, 5, 7, E.R - 1] + [rng.randrange(1, E.R) for _ in range(10)]
    g1 = [None]
    g2 = [None]
    for k in ks:
        p, q = E.mul(E.G1, k), E.g2_mul(E.G2, k)
        g1 += [p, E.neg(p)]
        g2 += [q, g2neg(q)]
    return g1, g2


def proofs_of(g1, g2):
    n = max(len(g1), len(g2))
    return [(g1[i % len(g1)], g2[i % len(g2)], g1[(3 * i + 1) % len(g1)]) for i in range(n)]


def test_the_symbols_exist_and_the_header_declares_them():
    lib = frw.load_library()
    text = open(os.path.join(ROOT, "include", "frw.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\(" % name, text), name
    assert "#define FRW_WIRE_COMPRESSED 0" in re.sub(r" +", " ", text) and "#define FRW_WIRE_UNCOMPRESSED 1" in re.sub(r" +", " ", text)
    assert [lib.frw_groth16_proof_wire_bytes(m) for m in (0, 1, 2, -1)] == [192, 384, 0, 0]
    assert [lib.frw_groth16_vk_wire_bytes(n, m) for n, m in ((1, 0), (3, 0), (3, 1), (3, 2))] == [344 + 48, 344 + 144, 680 + 288, 0]
    assert frw.WIRE_COMPRESSED == 0 and frw.WIRE_UNCOMPRESSED == 1


def test_the_codecs_constants():
    """frw_wire.h: 2^812 mod q, 2^-1 x 2^406 mod q, (q - 1) / 2, (q + 1) / 4 -- and the arithmetic facts the format's description leans on"""
    text = open(os.path.join(ROOT, "falcon-r1cs_amd", "csrc", "frw_wire.h")).read()

    def words(name, bits):
        body = re.search(r"%s(?:\[12\])? = \{+([^}]*)\}" % name, text).group(1)
        return sum(int(w.strip().rstrip("u"), 16) << (bits * i) for i, w in enumerate(body.split(",")))
    assert words("FQ29_R2", 29) == (1 << 812) % Q
    assert words("FQ29_HALF", 29) == pow(2, -1, Q) * (1 << 406) % Q
    assert words("Q_HALF32", 32) == (Q - 1) // 2
    assert words("SQRT_EXP32", 32) == (Q + 1) // 4 and ((Q + 1) // 4).bit_length() == int(re.search(r"SQRT_EXP_BITS = (\d+)", text).group(1))
    assert Q % 4 == 3
    assert W.fq_sqrt(5) is None                                              # x = 1 has no y on G1
    assert not W.fq_greater(E.G1[1])                                          # the generator's y is the smaller one
    assert W.g1_encode(E.G1)[47] & 0xC0 == 0


@pytest.mark.parametrize("compressed", MODES)
def test_encoding_equals_the_restatement_byte_for_byte(compressed):
    g1, g2 = points()
    # the set holds both values of bit 7 for G1 and for G2, and the c1-decided branch of the Fq2 order both ways
    assert {W.fq_greater(p[1]) for p in g1 if p} == {True, False}
    assert {W.fq2_greater(p[1]) for p in g2 if p} == {True, False}
    assert all(p[1][1] != 0 for p in g2 if p)
    cases = proofs_of(g1, g2)
    limbs = np.stack([proof_limbs(c) for c in cases])
    got, st = frw.proofs_to_wire(limbs, compressed)
    assert st.tolist() == [0] * len(cases)
    for i, c in enumerate(cases):
        assert got[i].tobytes() == W.proof_encode(c, compressed), i
    assert got.shape[1] == (192 if compressed else 384)
    if compressed:
        tops = [int(got[i, 47]) & 0xC0 for i in range(len(cases))]
        assert {0x00, 0x80, 0x40} == set(tops)
        assert {0x00, 0x80, 0x40} == {int(got[i, 48 + 95]) & 0xC0 for i in range(len(cases))}
    # the c1-equal branch: y.c1 = 0 leaves the order to c0.  The encoder does not ask whether a point is on its curve, so a made-up
    # "point" with y = (c0, 0) goes through it; the comparator is also asked directly (frw_diag_wire_greater)
    rng = random.Random(9)
    for c0 in (1, (Q - 1) // 2, (Q + 1) // 2, Q - 1, rng.randrange(Q)):
        fake = ((rng.randrange(Q), rng.randrange(Q)), (c0, 0))
        one = proof_limbs((E.G1, fake, E.G1))[None]
        out, st = frw.proofs_to_wire(one, compressed)
        assert st.tolist() == [0] and out[0].tobytes() == W.proof_encode((E.G1, fake, E.G1), compressed), c0
    # a coordinate >= q is refused, its bytes are zero, the neighbours stand
    bad = limbs[:3].copy()
    v = int.from_bytes(bad[1, 12:18].tobytes(), "little") + Q
    bad[1, 12:18] = np.frombuffer(v.to_bytes(48, "little"), dtype=np.uint64)
    out, st = frw.proofs_to_wire(bad, compressed)
    assert st.tolist() == [0, -1, 0] and not out[1].any()
    assert out[0].tobytes() == got[0].tobytes() and out[2].tobytes() == got[2].tobytes()


def test_the_order_of_fq_and_fq2_at_the_comparator():
    lib = frw.load_library()
    rng = random.Random(77)

    def w(v):
        return u64([(v >> (64 * i)) & (2 ** 64 - 1) for i in range(6)])
    fq = [0, 1, (Q - 1) // 2, (Q + 1) // 2, Q - 1] + [rng.randrange(Q) for _ in range(20)]
    for y in fq:
        assert lib.frw_diag_wire_greater(w(y).ctypes.data_as(C.c_void_p), None) == int(W.fq_greater(y)), y
    seen = set()
    for c1 in [0, 0, 0, 1, (Q - 1) // 2, (Q + 1) // 2, Q - 1] + [rng.randrange(Q) for _ in range(10)]:
        for c0 in fq:
            got = lib.frw_diag_wire_greater(w(c0).ctypes.data_as(C.c_void_p), w(c1).ctypes.data_as(C.c_void_p))
            assert got == int(W.fq2_greater((c0, c1))), (c0, c1)
            seen.add((c1 == 0, bool(got)))
    assert seen == {(True, True), (True, False), (False, True), (False, False)}     # both branches of c1-then-c0, both answers
    assert lib.frw_diag_wire_greater(None, None) == -1


def _g2_x_without_root():
    k = 0
    while True:
        k += 1
        x = (k, 0)
        if W.fq2_sqrt(E.f2_add(E.f2_mul(E.f2_mul(x, x), x), (4, 4))) is None:
            return x


def malformed_cases(compressed, good):
    """name -> one proof's bytes, made malformed in exactly one way from `good` (a valid proof's bytes)"""
    n1, n2 = W.g1_len(compressed), W.g2_len(compressed)
    top_a, top_b, top_c = n1 - 1, n1 + n2 - 1, 2 * n1 + n2 - 1        # the byte that carries each point's flags

    def put(at, chunk):
        b = bytearray(good)
        b[at:at + len(chunk)] = chunk
        return bytes(b)

    def flag(at, bits):
        b = bytearray(good)
        b[at] |= bits
        return bytes(b)
    fq = lambda v: v.to_bytes(48, "little")
    cases = {"A: x >= q": put(0, fq(Q)), "A: x = q + 1": put(0, fq(Q + 1)), "B: x.c0 >= q": put(n1, fq(Q + 5)), "B: x.c1 >= q": put(n1 + 48, fq(Q)),
             "C: x >= q": put(n1 + n2, fq(Q)), "A: bit 5 of the top byte": put(0, fq((1 << 381) + 1)),
             "A: both flags": flag(top_a, 0xC0), "B: both flags": flag(top_b, 0xC0), "C: both flags": flag(top_c, 0xC0),
             "A: infinity with a non-zero x": flag(top_a, 0x40) if not compressed else put(0, W._fq(E.G1[0], 0x40)),
             "B: infinity with a non-zero x": put(n1, W._fq2(E.G2[0], 0x40)) if compressed else flag(top_b, 0x40)}
    if compressed:
        cases["A: x = 1 has no y"] = put(0, fq(1))
        cases["C: x = 1 has no y, bit 7 set"] = put(n1 + n2, W._fq(1, 0x80))
        cases["B: an x with no y"] = put(n1, W._fq2(_g2_x_without_root()))
    else:
        cases["A: y >= q"] = put(48, fq(Q + 2))
        cases["A: off the curve"] = put(48, fq((E.G1[1] + 1) % Q))
        cases["B: off the curve"] = put(n1 + 96, fq((E.G2[1][0] + 1) % Q))
        cases["C: off the curve"] = put(n1 + n2, fq(1))
        cases["A: bit 7 in an uncompressed point"] = flag(top_a, 0x80)
        cases["B: bit 7 in an uncompressed point"] = flag(top_b, 0x80)
        cases["A: infinity with a non-zero y"] = put(0, fq(0) + W._fq(2, 0x40))
        cases["B: x.c0 carries flag bits"] = flag(n1 + 47, 0x80)
    for name, b in cases.items():                                          # the restatement refuses every one of them
        with pytest.raises(W.Malformed):
            W.proof_decode(b, compressed)
    return cases


@pytest.mark.parametrize("compressed", MODES)
def test_decoding_inverts_encoding_and_refuses_every_malformed_case(compressed):
    g1, g2 = points()
    cases = proofs_of(g1, g2)
    limbs = np.stack([proof_limbs(c) for c in cases])
    wire = np.stack([np.frombuffer(W.proof_encode(c, compressed), dtype=np.uint8) for c in cases])
    back, st = frw.proofs_from_wire(wire, compressed)
    assert st.tolist() == [0] * len(cases)
    assert np.array_equal(back, limbs)
    # bytes at an odd address decode the same
    shifted = np.zeros(wire.size + 1, dtype=np.uint8)
    shifted[1:] = wire.reshape(-1)
    back2, st2 = frw.proofs_from_wire(shifted[1:].reshape(wire.shape), compressed)
    assert np.array_equal(back2, limbs) and not st2.any()
    # every malformed case alone in a valid batch: -1 and zero limbs there, the neighbours untouched
    good = W.proof_encode((E.G1, E.G2, E.mul(E.G1, 9)), compressed)
    for name, b in malformed_cases(compressed, good).items():
        batch = wire[:5].copy()
        batch[2] = np.frombuffer(b, dtype=np.uint8)
        out, st = frw.proofs_from_wire(batch, compressed)
        assert st.tolist() == [0, 0, -1, 0, 0], name
        assert not out[2].any(), name
        assert np.array_equal(out[[0, 1, 3, 4]], limbs[[0, 1, 3, 4]]), name
    # bad arguments
    lib = frw.load_library()
    p = wire.ctypes.data_as(C.c_void_p)
    assert lib.frw_groth16_proofs_from_wire(1, p, 2, p, p) == -1 and lib.frw_groth16_proofs_to_wire(1, p, -1, p, p) == -1
    assert lib.frw_groth16_proofs_from_wire(1, None, 0, p, p) == -1 and lib.frw_groth16_proofs_to_wire(1, p, 0, None, p) == -1
    assert lib.frw_groth16_proofs_from_wire(1, p, 0, p, None) == -1


def g2_points_whose_y_squared_has_no_u_part():
    """The Fq2 root's a1 = 0 branch, which random points never reach: x = (s, t) with s^2 = (t^3 - 4) / (3 t) makes the u part of
    x^3 + 4 (1 + u) vanish, so y^2 = a lies in Fq and y is (sqrt(a), 0) or (0, sqrt(-a)) -- a residue and a non-residue, both signs of y.
    (Points of the curve, not of the subgroup: that is not the codec's business.)"""
    pts = []
    for t in range(1, 40):
        s = W.fq_sqrt((t ** 3 - 4) * pow(3 * t, -1, Q) % Q)
        if s is None:
            continue
        for x in ((s, t), (Q - s, t)):
            rhs = E.f2_add(E.f2_mul(E.f2_mul(x, x), x), (4, 4))
            assert rhs[1] == 0 and rhs[0] != 0
            r = W.fq_sqrt(rhs[0])
            y = (r, 0) if r is not None else (0, W.fq_sqrt(Q - rhs[0]))
            assert E.f2_mul(y, y) == rhs
            pts += [(x, y), g2neg((x, y))]
    return pts


def test_g2_points_whose_y_squared_has_no_u_part():
    pts = g2_points_whose_y_squared_has_no_u_part()
    kinds = {(p[1][1] == 0, W.fq2_greater(p[1])) for p in pts}
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}    # a residue or not, the greater y or not
    cases = [(E.G1, p, E.mul(E.G1, 3)) for p in pts]
    limbs = np.stack([proof_limbs(c) for c in cases])
    for compressed in MODES:
        wire = np.stack([np.frombuffer(W.proof_encode(c, compressed), dtype=np.uint8) for c in cases])
        got, st = frw.proofs_to_wire(limbs, compressed)
        assert not st.any() and np.array_equal(got, wire)
        back, st = frw.proofs_from_wire(wire, compressed)
        assert st.tolist() == [0] * len(cases)
        assert np.array_equal(back, limbs)


def _vk_flat(vk):
    d = vk_limbs(vk)
    return np.concatenate([d[k].reshape(-1) for k in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1")])


@pytest.mark.parametrize("compressed", MODES)
def test_keys_round_trip_and_bad_buffers_are_refused(compressed):
    rng = random.Random(55)
    vk, x, proof = make_statement(rng, 2, 14)                               # num_instance 3
    want = W.vk_encode(vk, compressed)
    assert len(want) == (344 + 48 * 3 if compressed else 680 + 96 * 3)
    got = frw.vk_to_wire(vk_limbs(vk), compressed)
    assert got == want
    assert frw.vk_to_wire(_vk_flat(vk), compressed) == want
    ver = frw.Groth16Verifier.from_wire(got, compressed=compressed)
    assert ver.num_instance == 3
    inst = fr_limbs(x, True)[None]
    assert ver.verify(inst, proof_limbs(proof)[None]).tolist() == [1]
    assert ver.verify(inst, proof_limbs((proof[0], proof[1], E.add(proof[2], E.G1)))[None]).tolist() == [0]
    ver.close()
    lib = frw.load_library()
    head = 336 if compressed else 672
    g1n = W.g1_len(compressed)

    def load(b, mode=None):
        h = C.c_void_p(99)
        buf = (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b or b"\0")
        rc = lib.frw_groth16_vk_load_wire(buf, len(b), (0 if compressed else 1) if mode is None else mode, C.byref(h))
        if rc == 0:
            lib.frw_groth16_vk_free(h)
        else:
            assert not h.value
        return rc
    assert load(want) == 0
    assert load(want[:-1]) == -1 and load(want[:-g1n]) == -1 and load(want[:head + 4]) == -1 and load(b"") == -1      # truncated
    assert load(want + b"\0") == -1 and load(want + want[-g1n:]) == -1                                                # over-long
    for n in (0, 2, 4, 1 << 40, 2 ** 64 - 1):                                                                           # n does not match
        assert load(want[:head] + n.to_bytes(8, "little") + want[head + 8:]) == -1, n
    assert load(want, 2) == -1
    # one bad gamma_abc_g1 row; one bad fixed point
    bad_row = W._fq(1) if compressed else W._fq(E.G1[0]) + W._fq((E.G1[1] + 1) % Q)
    assert load(want[:head + 8 + g1n] + bad_row + want[head + 8 + 2 * g1n:]) == -1
    assert load(want[:g1n + 47] + bytes([want[g1n + 47] | 0xC0]) + want[g1n + 48:]) == -1
    with pytest.raises(frw.FrwError) as ei:
        frw.Groth16Verifier.from_wire(want[:-1], compressed=compressed)
    assert ei.value.code == -1
    # the encoder refuses limbs >= q and num_instance = 0
    flat = _vk_flat(vk).copy()
    out = np.zeros(len(want), dtype=np.uint8)
    assert lib.frw_groth16_vk_to_wire(flat.ctypes.data_as(C.c_void_p), 0, 0 if compressed else 1, out.ctypes.data_as(C.c_void_p)) == -1
    flat[84 + 12:84 + 18] = np.frombuffer((int.from_bytes(flat[84 + 12:84 + 18].tobytes(), "little") + Q).to_bytes(48, "little"), dtype=np.uint64)
    assert lib.frw_groth16_vk_to_wire(flat.ctypes.data_as(C.c_void_p), 3, 0 if compressed else 1, out.ctypes.data_as(C.c_void_p)) == -1


@pytest.mark.parametrize("compressed", MODES)
def test_a_proof_verifies_after_a_trip_through_the_wire(compressed):
    rng = random.Random(66)
    vk, x, proof = make_statement(rng, 3, 14)
    ver = frw.Groth16Verifier(vk_limbs(vk))
    inst = fr_limbs(x, True)[None]
    limbs = proof_limbs(proof)[None]
    assert ver.verify(inst, limbs).tolist() == [1]
    wire, st = frw.proofs_to_wire(limbs, compressed)
    assert st.tolist() == [0] and wire[0].tobytes() == W.proof_encode(proof, compressed)
    back, st = frw.proofs_from_wire(wire.tobytes(), compressed)
    assert st.tolist() == [0] and np.array_equal(back, limbs)
    assert ver.verify(inst, back).tolist() == [1]
    if compressed:
        # bit 7 of A flipped: -A, a valid point and another proof
        flipped = wire.copy()
        flipped[0, 47] ^= 0x80
        other, st = frw.proofs_from_wire(flipped, True)
        assert st.tolist() == [0]
        assert np.array_equal(other[0], proof_limbs((E.neg(proof[0]), proof[1], proof[2])))
        assert ver.verify(inst, other).tolist() == [0]
    ver.close()


def test_dev_entry_points_without_a_device_and_with_bad_arguments():
    """a device index that no machine has: FRW_E_NO_DEVICE, never a host fallback; null pointers and a bad mode: FRW_E_INVALID_ARG first"""
    lib = frw.load_library()
    nowhere = 1 << 20
    buf = np.zeros(4096, dtype=np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    for mode in (0, 1):
        assert lib.frw_groth16_proofs_to_wire_dev(nowhere, 1, p, mode, p, p, None) == -2
        assert lib.frw_groth16_proofs_from_wire_dev(nowhere, 1, p, mode, p, p, None) == -2
    for fn in (lib.frw_groth16_proofs_to_wire_dev, lib.frw_groth16_proofs_from_wire_dev):
        assert fn(nowhere, 1, p, 2, p, p, None) == -1
        assert fn(nowhere, 1, None, 0, p, p, None) == -1 and fn(nowhere, 1, p, 0, None, p, None) == -1 and fn(nowhere, 1, p, 0, p, None, None) == -1
    rng = random.Random(3)
    vk, _, _ = make_statement(rng, 2, 14)
    h = C.c_void_p(5)
    for compressed in MODES:
        key = W.vk_encode(vk, compressed)
        kb = (C.c_uint8 * len(key)).from_buffer_copy(key)
        mode = 0 if compressed else 1
        assert lib.frw_groth16_vk_load_wire_dev(nowhere, kb, len(key), mode, C.byref(h)) == -2 and not h.value
        assert lib.frw_groth16_vk_load_wire_dev(nowhere, kb, len(key) - 1, mode, C.byref(h)) == -1
        assert lib.frw_groth16_vk_load_wire_dev(nowhere, kb, len(key), 2, C.byref(h)) == -1
        assert lib.frw_groth16_vk_load_wire_dev(nowhere, None, len(key), mode, C.byref(h)) == -1
        assert lib.frw_groth16_vk_load_wire_dev(nowhere, kb, len(key), mode, None) == -1
        with pytest.raises(frw.FrwError) as ei:
            frw.Groth16Verifier.from_wire(key, device=nowhere, compressed=compressed)
        assert ei.value.code == -2
    # verification from wire bytes needs a key with a device part: a host key and a null key are refused before any device is touched
    host = frw.Groth16Verifier(vk_limbs(vk))
    acc = np.zeros(1, dtype=np.int32)
    for keyh in (host._h, None):
        assert lib.frw_groth16_verify_wire_workspace_bytes(keyh, 1, 0, 0) == 0
        assert lib.frw_groth16_verify_wire_dev(keyh, 1, p, frw.ENC_MONTGOMERY, p, 0, 0, None, acc.ctypes.data_as(C.c_void_p), None, p, 4096, None) == -1
    host.close()
