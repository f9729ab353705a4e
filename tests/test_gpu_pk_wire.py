"""Groth16 PROVING keys in ark-serialize's wire format on the device (frw_groth16_pk_load_wire_dev / frw_groth16_pk_to_wire_dev): a key
loaded from the bytes tests/pk_wire_ref.py wrote (Python integers, from the format table) against the same key loaded from limbs, sum
for sum over each of the five queries; the export of the limb-loaded handle against those bytes, byte for byte; one corrupted point
per refusal; and a Falcon-512 key written, read back and proved with.

The keys belong to no circuit (frw_groth16_pk_load_opts takes any counts): random multiples of the generators, with the points at
infinity a real key is full of.  Shapes: the smallest whose every run crosses a 64-lane boundary --
  S: I = 3, W = 30, n = 64     33 + 3 witness-side rows, 63 h_query points
  M: I = 5, W = 124, n = 128   129 + 3 rows, 127 points."""
import random

import numpy as np
import pytest

import frw_testlib as T
import pk_wire_ref as P
import wire_ref as W
from oracle import bls12_381 as E

pytestmark = pytest.mark.gpu
R, Q = E.R, E.Q
SHAPES = {"S": (3, 30, 64), "M": (5, 124, 128)}
_KEYS = {}
_WIRE = {}


def make_key(engine, shape):
    """(limbs: dict of uint64 arrays in ark-ff's form, points: the same key as Python integers for pk_wire_ref), made once per shape"""
    if shape in _KEYS:
        return _KEYS[shape]
    ni, nw, n = SHAPES[shape]
    nv = ni + nw
    rng = random.Random(5000 + n)
    g1 = engine.g1_fixed_base(T.ints_to_limbs([rng.randrange(1, R) for _ in range(3 + ni + 2 * nv + (n - 1) + nw)]))
    g2 = engine.g2_fixed_base(T.ints_to_limbs([rng.randrange(1, R) for _ in range(3 + nv)]))
    cut, pos = {}, 3
    for name, count in (("gamma_abc_g1", ni), ("a_query", nv), ("b_g1_query", nv), ("h_query", n - 1), ("l_query", nw)):
        cut[name] = g1[pos:pos + count].copy()
        pos += count
    cut["b_g2_query"] = g2[3:].copy()
    # a third of b_g1_query / b_g2_query, at the same indices: variables on no B side; a few of a_query, first and last included
    for i in range(nv):
        if i % 3 == 1:
            cut["b_g1_query"][i] = 0
            cut["b_g2_query"][i] = 0
    for i in (0, 17, nv // 2, nv - 1):
        cut["a_query"][i] = 0
    limbs = dict(cut, alpha_g1=g1[0].copy(), beta_g1=g1[1].copy(), delta_g1=g1[2].copy(), beta_g2=g2[0].copy(), gamma_g2=g2[1].copy(),
                 delta_g2=g2[2].copy())
    p1 = lambda rows: [E.from_limbs(r) for r in rows]
    p2 = lambda rows: [E.g2_from_limbs(r) for r in rows]
    points = {"vk": {"alpha_g1": E.from_limbs(limbs["alpha_g1"]), "beta_g2": E.g2_from_limbs(limbs["beta_g2"]),
                     "gamma_g2": E.g2_from_limbs(limbs["gamma_g2"]), "delta_g2": E.g2_from_limbs(limbs["delta_g2"]),
                     "gamma_abc_g1": p1(limbs["gamma_abc_g1"])},
              "beta_g1": E.from_limbs(limbs["beta_g1"]), "delta_g1": E.from_limbs(limbs["delta_g1"]),
              "a_query": p1(limbs["a_query"]), "b_g1_query": p1(limbs["b_g1_query"]), "b_g2_query": p2(limbs["b_g2_query"]),
              "h_query": p1(limbs["h_query"]), "l_query": p1(limbs["l_query"])}
    _KEYS[shape] = (limbs, points)
    return _KEYS[shape]


def wire_of(engine, shape, compressed):
    if (shape, compressed) not in _WIRE:
        _WIRE[shape, compressed] = P.pk_encode(make_key(engine, shape)[1], compressed)
    return _WIRE[shape, compressed]


def load_limbs(engine, shape, mode):
    ni, nw, n = SHAPES[shape]
    k = make_key(engine, shape)[0]
    return engine.groth16_pk_load(ni, nw, n, k["alpha_g1"], k["beta_g1"], k["delta_g1"], k["beta_g2"], k["delta_g2"], k["a_query"],
                                  k["b_g1_query"], k["b_g2_query"], k["h_query"], k["l_query"], mode=mode)


def vk_limbs(limbs):
    return {name: limbs[name] for name in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1")}


def _sum(engine, handle, scalars, g2):
    """one scalar vector (uint64[count, 4], canonical) through frw_msm_g1_dev / frw_msm_g2_dev -> the affine sum's limbs"""
    import torch
    dev = torch.device("cuda:0")
    info = engine.msm_info(handle)
    assert int(info.num_points) == scalars.shape[0]
    d_sc = torch.from_numpy(scalars.view(np.int64)).to(dev)
    out = torch.full((1, 24 if g2 else 12), -1, dtype=torch.int64, device=dev)
    ws = torch.empty(int(info.workspace_bytes_per_signature), dtype=torch.uint8, device=dev)
    fn = engine.msm_g2_dev if g2 else engine.msm_g1_dev
    fn(handle, 1, d_sc, scalars.shape[0], 0, out, ws, ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)[0]


@pytest.mark.parametrize("mode", ["tables", "bare"])
@pytest.mark.parametrize("compressed", [True, False], ids=["compressed", "uncompressed"])
@pytest.mark.parametrize("shape", ["S", "M"])
def test_a_key_from_wire_bytes_equals_the_key_from_limbs(engine, shape, compressed, mode):
    import falcon_r1cs_amd as frw
    key_mode = frw.KEY_TABLES if mode == "tables" else frw.KEY_BARE
    ni, nw, n = SHAPES[shape]
    limbs = make_key(engine, shape)[0]
    data = wire_of(engine, shape, compressed)
    assert len(data) == engine.groth16_pk_wire_bytes(ni, nw, n, compressed)
    got, vk = engine.groth16_pk_load_wire(data, compressed=compressed, checked=True, mode=key_mode)
    want = load_limbs(engine, shape, key_mode)
    try:
        a, b = engine.groth16_pk_info(got), engine.groth16_pk_info(want)
        for field in ("mode", "rank", "world", "z_lo", "z_hi", "h_lo", "h_hi", "key_bytes"):
            assert getattr(a, field) == getattr(b, field), field
        assert a.mode == key_mode and (a.z_hi, a.h_hi) == (ni + nw + 3, n - 1)
        rng = random.Random(77)
        for which in range(5):                                                   # h_query, a_query, b_g1_query, l_query, b_g2_query
            count = n - 1 if which == 0 else ni + nw + 3
            ks = [rng.randrange(R) for _ in range(count)]
            ks[1], ks[2], ks[count - 2] = 0, 1, 1
            sc = T.ints_to_limbs(ks)
            mine = _sum(engine, engine.groth16_pk_query(got, which), sc, which == 4)
            theirs = _sum(engine, engine.groth16_pk_query(want, which), sc, which == 4)
            assert mine.any() and np.array_equal(mine, theirs), which
        for name, value in vk_limbs(limbs).items():
            assert np.array_equal(np.asarray(vk[name]).reshape(-1), value.reshape(-1)), name
    finally:
        engine.groth16_pk_free(got)
        engine.groth16_pk_free(want)


@pytest.mark.parametrize("mode", ["tables", "bare"])
@pytest.mark.parametrize("compressed", [True, False], ids=["compressed", "uncompressed"])
@pytest.mark.parametrize("shape", ["S", "M"])
def test_the_export_of_a_limb_loaded_key_equals_the_restatement(engine, shape, compressed, mode):
    import falcon_r1cs_amd as frw
    limbs = make_key(engine, shape)[0]
    pk = load_limbs(engine, shape, frw.KEY_TABLES if mode == "tables" else frw.KEY_BARE)
    try:
        got = engine.groth16_pk_to_wire(pk, vk_limbs(limbs), compressed=compressed)
        want = wire_of(engine, shape, compressed)
        assert len(got) == len(want)
        assert got == want, next(i for i in range(len(want)) if got[i] != want[i])
        # the wrong size, the wrong instance count
        lib = frw.load_library()
        import ctypes as C
        flat = np.concatenate([v.reshape(-1) for v in vk_limbs(limbs).values()])
        out = np.zeros(len(want) + 1, dtype=np.uint8)
        args = (pk, flat.ctypes.data_as(C.c_void_p), SHAPES[shape][0], 0 if compressed else 1, out.ctypes.data_as(C.c_void_p))
        assert lib.frw_groth16_pk_to_wire_dev(*args, len(want) + 1) == -1 and lib.frw_groth16_pk_to_wire_dev(*args, len(want) - 1) == -1
        assert lib.frw_groth16_pk_to_wire_dev(args[0], args[1], SHAPES[shape][0] - 1, args[3], args[4], len(want)) == -1
    finally:
        engine.groth16_pk_free(pk)


def _ladder(add, p, k):
    """k P without reducing k modulo the group order (oracle/bls12_381.py's mul does reduce)"""
    acc = None
    while k:
        if k & 1:
            acc = add(acc, p)
        p = add(p, p)
        k >>= 1
    return acc


def _off_subgroup_g1():
    for x in range(1, 200):
        y = W.fq_sqrt((x * x * x + 4) % Q)
        if y is not None and _ladder(E.add, (x, y), R) is not None:
            return (x, y)
    raise AssertionError("no G1 point outside the subgroup among the small x")


def _off_subgroup_g2():
    for c in range(1, 200):
        x = (c, 0)
        y = W.fq2_sqrt(E.f2_add(E.f2_mul(E.f2_mul(x, x), x), (4, 4)))
        if y is not None and _ladder(E.g2_add, (x, y), R) is not None:
            return (x, y)
    raise AssertionError("no point of the twist outside the subgroup among the small x")


def _corrupted(engine):
    """name -> (compressed, the shape-S bytes with ONE point replaced, what frw_last_error must name, loads when vouched for)"""
    ni, nw, n = SHAPES["S"]
    nv = ni + nw
    points = make_key(engine, "S")[1]
    cases = {}

    def patch(compressed, query, index, new):
        data = bytearray(wire_of(engine, "S", compressed))
        off = P.pk_offsets(points, compressed)[query] + index * len(new)
        assert len(new) == (W.g2_len(compressed) if query == "b_g2_query" else W.g1_len(compressed))
        data[off:off + len(new)] = new
        return bytes(data)
    no_root = next(x for x in range(1, 100) if W.fq_sqrt((x * x * x + 4) % Q) is None)
    cases["no root"] = (True, patch(True, "h_query", 62, no_root.to_bytes(48, "little")), "h_query[62]", False)
    cases["coordinate >= q"] = (True, patch(True, "a_query", 0, Q.to_bytes(48, "little")), "a_query[0]", False)
    live = next(i for i in range(nv) if points["b_g1_query"][i] is not None and i > 2)
    both = bytearray(W.g1_encode(points["b_g1_query"][live], True))
    both[47] |= 0xC0
    cases["both flags"] = (True, patch(True, "b_g1_query", live, bytes(both)), "b_g1_query[%d]" % live, False)
    x, y = points["b_g2_query"][live]
    off_curve = (x, ((y[0] + 1) % Q, y[1]))
    assert not E.g2_on_curve(off_curve)
    cases["off the twist"] = (False, patch(False, "b_g2_query", live, W.g2_encode(off_curve, False)), "b_g2_query[%d]" % live, False)
    stray1, stray2 = _off_subgroup_g1(), _off_subgroup_g2()
    assert E.on_curve(stray1) and _ladder(E.add, stray1, R) is not None
    assert E.g2_on_curve(stray2) and _ladder(E.g2_add, stray2, R) is not None
    cases["G1 outside the subgroup"] = (True, patch(True, "l_query", nw - 1, W.g1_encode(stray1, True)), "l_query[%d]" % (nw - 1), True)
    cases["G2 outside the subgroup"] = (True, patch(True, "b_g2_query", live, W.g2_encode(stray2, True)), "b_g2_query[%d]" % live, True)
    return cases


CASES = ["no root", "coordinate >= q", "both flags", "off the twist", "G1 outside the subgroup", "G2 outside the subgroup"]


@pytest.mark.parametrize("case", CASES)
def test_one_bad_point_refuses_the_key(engine, case):
    import falcon_r1cs_amd as frw
    compressed, data, named, loads_when_vouched = _corrupted(engine)[case]
    assert engine.groth16_pk_wire_info(data, compressed)["num_instance"] == 3          # (the framing is intact)
    for mode in (frw.KEY_TABLES, frw.KEY_BARE):
        with pytest.raises(frw.FrwError) as ei:
            engine.groth16_pk_load_wire(data, compressed=compressed, checked=True, mode=mode)
        assert ei.value.code == -1 and named in str(ei.value), str(ei.value)
    # vouching skips the subgroup ladder and nothing else
    if loads_when_vouched:
        pk, _ = engine.groth16_pk_load_wire(data, compressed=compressed, checked=False)
        engine.groth16_pk_free(pk)
    else:
        with pytest.raises(frw.FrwError) as ei:
            engine.groth16_pk_load_wire(data, compressed=compressed, checked=False)
        assert ei.value.code == -1 and named in str(ei.value), str(ei.value)


def test_a_falcon_512_key_written_and_read_back_proves_the_same(engine):
    """setup -> bytes -> load: both handles give byte-equal proofs for the same blinding factors, and a verifier made from the LOADED
    key's verifying key accepts them -- and rejects them for a statement with one public input changed"""
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    logn, batch = 9, 2
    L = frw.layout(logn)
    rng = random.Random(909)
    pk, vk = engine.groth16_setup(0, logn, *(rng.randrange(2, R) for _ in range(5)))
    pk2 = r1cs = None
    try:
        data = engine.groth16_pk_to_wire(pk, vk, compressed=True)
        info = engine.groth16_pk_wire_info(data, True)
        assert (info["num_instance"], info["num_witness"]) == (L.num_instance, L.num_witness)
        pk2, vk2 = engine.groth16_pk_load_wire(data, compressed=True, checked=True)
        for name in vk:
            assert np.array_equal(np.asarray(vk[name]), np.asarray(vk2[name])), name
        r1cs = engine.r1cs_load(0, logn)
        sig, pk_, hm = frw.synth_triples(logn, batch, seed=61)
        dd = [torch.from_numpy(a.view(np.int16)).to(dev) for a in (sig, pk_, hm)]
        wit = torch.empty((batch, L.num_witness, 4), dtype=torch.int64, device=dev)
        inst = torch.empty((batch, L.num_instance, 4), dtype=torch.int64, device=dev)
        st = torch.empty(batch, dtype=torch.int32, device=dev)
        s0 = torch.cuda.current_stream().cuda_stream
        engine.witness_ntt_verify_dev(logn, batch, dd[0], dd[1], dd[2], wit, inst, st, frw.ENC_MONTGOMERY, s0)
        rs = np.array([T.ints_to_limbs([rng.randrange(R), rng.randrange(R)]) for _ in range(batch)])
        proofs = []
        for key in (pk, pk2):
            ws_bytes = engine.groth16_workspace_bytes(key, r1cs, batch)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            out = torch.zeros((batch, 48), dtype=torch.int64, device=dev)
            bad = torch.empty(batch, dtype=torch.int32, device=dev)
            engine.groth16_prove_dev(key, r1cs, batch, wit, inst, rs, out, ws, ws_bytes, bad, s0)
            torch.cuda.synchronize()
            assert bad.tolist() == [0] * batch
            proofs.append(out.cpu().numpy().view(np.uint64))
        assert proofs[0].any() and np.array_equal(proofs[0], proofs[1])
        verifier = frw.Groth16Verifier(vk2)
        try:
            instance = inst.cpu().numpy().view(np.uint64)
            assert verifier.verify(instance, proofs[1]).tolist() == [1] * batch
            other = instance.copy()
            other[:, 5] = other[:, 6]                                            # one public input changed (still a field element)
            assert not np.array_equal(other, instance)
            assert verifier.verify(other, proofs[1]).tolist() == [0] * batch
        finally:
            verifier.close()
    finally:
        if r1cs is not None:
            engine.r1cs_free(r1cs)
        if pk2 is not None:
            engine.groth16_pk_free(pk2)
        engine.groth16_pk_free(pk)
