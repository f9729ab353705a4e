"""The prover from bytes on the device (frw_pok_prove_from_bytes_dev / frw_pok_prove_from_bytes): one call from encoded Falcon
signatures to Groth16 proofs on the wire, held to the chain of calls it replaces.

The reference of every comparison is that chain for ONE signature alone with the same blinding factors -- frw_prepare_inputs,
frw_witness_*_dev, frw_groth16_prove_rs_dev, frw_groth16_proofs_to_wire_dev, and frw_statement_from_bytes_dev for the instance vector --
computed once per (circuit, input) and shared by the tests (`chain`).  The contract under test: the bytes of slot i depend on slot i's
inputs and rs[i] alone, an accepted slot's are the chain's byte for byte, a refused slot's are zero in every output, and nothing is
written beyond the batch's entries (guard regions behind every output and behind the workspace).

Falcon-512 wherever the parameter set does not matter; one key and one constraint system per circuit for the whole module."""
import hashlib

import numpy as np
import pytest

import pok_prove_cases as PC

pytestmark = pytest.mark.gpu

NTT, DUAL, SCHOOLBOOK = 0, 1, 2
GUARD = 4096           # bytes of 0xA5 behind every output and behind the workspace


# ---- one key, one constraint system, one verifier per circuit ---------------------------------------------------------------------------
class Keys:
    def __init__(self, engine):
        self.engine, self.sets, self.chain_cache = engine, {}, {}

    def get(self, circuit, logn):
        import random
        import falcon_r1cs_amd as frw
        if (circuit, logn) not in self.sets:
            rng = random.Random(4100 + 10 * circuit + logn)
            key, vk = self.engine.groth16_setup(circuit, logn, *(rng.randrange(2, PC.R) for _ in range(5)))
            r1cs = self.engine.r1cs_load(circuit, logn)
            ver = frw.Groth16Verifier.from_wire(frw.vk_to_wire(vk), device=0)
            self.sets[(circuit, logn)] = (key, r1cs, ver)
        return self.sets[(circuit, logn)]

    def close(self):
        for key, r1cs, ver in self.sets.values():
            ver.close()
            self.engine.r1cs_free(r1cs)
            self.engine.groth16_pk_free(key)
        self.sets = {}


@pytest.fixture(scope="module")
def keys(engine):
    k = Keys(engine)
    yield k
    k.close()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def chain(keys, circuit, logn, triple, rs, compressed=True):
    """the existing calls for this signature alone -> dict(wire, proofs, instance) of numpy arrays; cached"""
    import torch
    import falcon_r1cs_amd as frw
    tag = (circuit, logn, hashlib.sha256(b"|".join(triple)).hexdigest(), rs.tobytes(), compressed)
    if tag in keys.chain_cache:
        return keys.chain_cache[tag]
    engine = keys.engine
    key, r1cs, _ = keys.get(circuit, logn)
    dev = torch.device("cuda:0")
    pkb, msg, sgb = triple
    sig, pk, hm, st = engine.prepare_inputs(logn, [pkb], [msg], [sgb])
    assert not st.any()
    L = frw.circuit_layout(circuit, logn)
    d = [torch.from_numpy(a.view(np.int16)).to(dev) for a in (sig, pk, hm)]
    wit = torch.empty((1, L.num_witness, 4), dtype=torch.int64, device=dev)
    inst = torch.empty((1, L.num_instance, 4), dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    witness = (engine.witness_ntt_verify_dev, engine.witness_dual_ntt_verify_dev, engine.witness_schoolbook_verify_dev)[circuit]
    witness(logn, 1, d[0], d[1], d[2], wit, inst, status, frw.ENC_MONTGOMERY, _stream())
    ws_bytes = engine.groth16_workspace_bytes(key, r1cs, 1)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    proof = torch.empty((1, 48), dtype=torch.int64, device=dev)
    bad = torch.empty(1, dtype=torch.int32, device=dev)
    d_rs = torch.from_numpy(rs.reshape(1, 2, 4).view(np.int64).copy()).to(dev)
    engine.groth16_prove_rs_dev(key, r1cs, 1, wit, inst, d_rs, proof, ws, ws_bytes, bad, _stream())
    wire, wire_status = frw.proofs_to_wire_dev(proof, compressed, _stream())
    inst2, st2 = engine.statement_from_bytes_dev(circuit, logn, [pkb], [sgb[1:1 + frw.NONCE_LEN]], [msg], frw.ENC_MONTGOMERY, _stream())
    torch.cuda.synchronize()
    assert status.tolist() == [0] and bad.tolist() == [0] and wire_status.tolist() == [0] and st2.tolist() == [0]
    assert torch.equal(inst2, inst)
    out = {"wire": wire[0].cpu().numpy(), "proofs": proof[0].cpu().numpy().view(np.uint64), "instance": inst2[0].cpu().numpy().view(np.uint64)}
    keys.chain_cache[tag] = out
    return out


# ---- the call under test, with guard regions --------------------------------------------------------------------------------------------
def _upload(logn, items):
    """items: [(triple, rs)] -> device tensors pk bytes, sig bytes, (blob, offsets), rs"""
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    up = lambda b: torch.from_numpy(np.frombuffer(b or b"\0", dtype=np.uint8).copy()).to(dev)
    pkb, msgs, sgb = (b"".join(t[k] for t, _ in items) for k in range(3))
    off = np.zeros(len(items) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(t[1]) for t, _ in items])
    rs = np.stack([r for _, r in items]) if items else np.zeros((1, 2, 4), dtype=np.uint64)
    assert all(len(t[0]) == frw.PK_LEN[logn] and len(t[2]) == frw.SIG_LEN[logn] for t, _ in items)
    return up(pkb), up(sgb), (up(msgs), torch.from_numpy(off).to(dev)), torch.from_numpy(rs.view(np.int64).copy()).to(dev)


def run(keys, circuit, logn, items, in_flight, compressed=True, want=(True, True, True)):
    """frw_pok_prove_from_bytes_dev through the raw entry point, every output and the workspace followed by GUARD bytes of 0xA5 that
    must come back untouched -> dict of numpy arrays (None where not asked for) and the status of frw_falcon_verify_from_bytes_dev"""
    import ctypes as C
    import torch
    import falcon_r1cs_amd as frw
    engine = keys.engine
    key, r1cs, _ = keys.get(circuit, logn)
    dev = torch.device("cuda:0")
    batch = len(items)
    d_pkb, d_sgb, (d_blob, d_off), d_rs = _upload(logn, items)
    wire_len = frw.proof_wire_bytes(compressed)
    I = (2 << logn) + 1
    sizes = {"wire": batch * wire_len, "proofs": batch * 384 if want[0] else None, "instance": batch * I * 32 if want[1] else None,
             "status": batch * 4, "num_unsatisfied": batch * 4 if want[2] else None}
    ws_bytes = engine.pok_prove_workspace_bytes(key, r1cs, circuit, logn, batch, in_flight)
    assert ws_bytes > 0 and ws_bytes % 16 == 0
    sizes["workspace"] = ws_bytes
    bufs = {k: torch.full((v + GUARD,), 0xA5, dtype=torch.uint8, device=dev) for k, v in sizes.items() if v is not None}
    assert all(b.data_ptr() % 256 == 0 for b in bufs.values())
    P = lambda k: C.c_void_p(bufs[k].data_ptr()) if k in bufs else None
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = engine._lib.frw_pok_prove_from_bytes_dev(engine._ctx, key, r1cs, circuit, logn, batch, p(d_pkb), p(d_sgb), frw.SIG_LEN[logn], p(d_blob),
                                                  p(d_off), p(d_rs), 0 if compressed else 1, P("wire"), P("proofs"), P("instance"),
                                                  P("status"), P("num_unsatisfied"), P("workspace"), ws_bytes, C.c_void_p(_stream()))
    torch.cuda.synchronize()
    assert rc == 0, (rc, engine._lib.frw_last_error())
    host = {k: b.cpu().numpy() for k, b in bufs.items()}
    for k, h in host.items():
        assert (h[sizes[k]:] == 0xA5).all(), "the guard region behind %s was written" % k
    out = {"wire": host["wire"][:sizes["wire"]].reshape(batch, wire_len),
           "proofs": host["proofs"][:sizes["proofs"]].view(np.uint64).reshape(batch, 48) if want[0] else None,
           "instance": host["instance"][:sizes["instance"]].view(np.uint64).reshape(batch, I, 4) if want[1] else None,
           "status": host["status"][:sizes["status"]].view(np.int32),
           "num_unsatisfied": host["num_unsatisfied"][:sizes["num_unsatisfied"]].view(np.uint32) if want[2] else None}
    if batch:
        ref, _ = engine.falcon_verify_from_bytes_dev(logn, d_pkb.reshape(batch, -1), d_sgb.reshape(batch, -1), (d_blob, d_off), frw.RULE_CIRCUIT,
                                                     _stream())
        torch.cuda.synchronize()
        assert out["status"].tolist() == ref.tolist()
    return out


def held_to_the_chain(keys, circuit, logn, items, out, want_status, compressed=True):
    """statuses as expected; accepted slots equal the chain's bytes; refused slots are zero everywhere; no violated rows anywhere"""
    assert out["status"].tolist() == want_status
    for i, ((triple, rs), st) in enumerate(zip(items, want_status)):
        if st == PC.OK:
            ref = chain(keys, circuit, logn, triple, rs, compressed)
            assert out["wire"][i].tobytes() == ref["wire"].tobytes(), "slot %d: wire bytes differ from the chain's" % i
            if out["proofs"] is not None:
                assert out["proofs"][i].tolist() == ref["proofs"].tolist(), "slot %d: limbs differ from the chain's" % i
            if out["instance"] is not None:
                assert np.array_equal(out["instance"][i], ref["instance"]), "slot %d: instance differs from the chain's" % i
        else:
            for name in ("wire", "proofs", "instance"):
                assert out[name] is None or not out[name][i].any(), "slot %d (refused): %s is not zero" % (i, name)
    if out["num_unsatisfied"] is not None:
        assert not out["num_unsatisfied"].any()


def verdicts(keys, circuit, logn, out, compressed=True):
    import torch
    dev = torch.device("cuda:0")
    _, _, ver = keys.get(circuit, logn)
    d_inst = torch.from_numpy(out["instance"].view(np.int64).copy()).to(dev)
    d_wire = torch.from_numpy(out["wire"].copy()).to(dev)
    v = ver.verify_wire_dev(d_inst, d_wire, compressed, stream=_stream())
    torch.cuda.synchronize()
    return v.tolist()


# ---- 1. the mixed batch -----------------------------------------------------------------------------------------------------------------
def mixed_items(logn=9):
    """nine slots: genuine, genuine, bad signature header, genuine, key coefficient >= q, genuine, norm exactly at the bound, genuine,
    genuine -- accepted and refused interleaved, the first and the last accepted.  The golden file has two genuine triples per parameter
    set; the other four are signed from its first key."""
    g = PC.genuine(logn, 6)
    triples = [g[0], g[1], PC.bad_header(g[2]), g[2], PC.bad_key(g[3]), g[3], PC.at_the_bound(logn), g[4], g[5]]
    status = [PC.OK, PC.OK, PC.DECODE, PC.OK, PC.DECODE, PC.OK, PC.NORM_BOUND, PC.OK, PC.OK]
    names = ["g0", "g1", "hdr", "g2", "key", "g3", "bound", "g4", "g5"]
    return [(t, PC.blinding(n)) for t, n in zip(triples, names)], status


@pytest.fixture(scope="module")
def mixed(keys):
    items, status = mixed_items()
    return items, status, {k: run(keys, NTT, 9, items, k) for k in (2, 9)}


@pytest.mark.parametrize("in_flight", [2, 9])
def test_mixed_batch_equals_the_chain_slot_by_slot(keys, mixed, in_flight):
    """in_flight = 2: chunks of 2, 2 and 2 accepted signatures that cross refused slots; 9: one chunk.  The same assertions for both."""
    items, status, outs = mixed
    out = outs[in_flight]
    held_to_the_chain(keys, NTT, 9, items, out, status)
    v = verdicts(keys, NTT, 9, out)
    assert [x == 1 for x in v] == [s == PC.OK for s in status], v
    assert all(x in (0, -1) for x, s in zip(v, status) if s != PC.OK)
    for name in ("wire", "proofs", "instance", "status", "num_unsatisfied"):
        assert np.array_equal(outs[2][name], outs[9][name]), name


# ---- 2. independence from the batch -----------------------------------------------------------------------------------------------------
def test_a_slot_s_bytes_do_not_depend_on_its_neighbours(keys, mixed):
    """the same nine inputs with slots 1 and 7 swapped (their blinding factors travel with them) and slot 3 refused as well: every
    input accepted both times has the bytes it had"""
    items, status, outs = mixed
    again = list(items)
    again[1], again[7] = items[7], items[1]
    again[3] = (PC.bad_header(items[3][0]), items[3][1])
    status2 = list(status)
    status2[3] = PC.DECODE
    out = run(keys, NTT, 9, again, 2)
    held_to_the_chain(keys, NTT, 9, again, out, status2)
    where = {0: 0, 1: 7, 7: 1, 5: 5, 8: 8}                      # slot now -> slot in the first run
    for now, before in where.items():
        for name in ("wire", "proofs", "instance"):
            assert np.array_equal(out[name][now], outs[2][name][before]), (name, now)


# ---- 3. the scan across wavefront and workgroup boundaries -----------------------------------------------------------------------------
def test_three_accepted_slots_in_a_batch_of_1030(keys):
    """slots 0, 64 and 1,029 genuine, every other one with a bad signature header: the scan's ranks cross a wavefront (64) and four
    workgroup boundaries (256 ..), the index list has three entries, three proofs are made"""
    g = PC.genuine(9, 3)
    refused = (PC.bad_header(g[0]), PC.blinding("refused"))
    items = [refused] * 1030
    status = [PC.DECODE] * 1030
    for slot, k in ((0, 0), (64, 1), (1029, 2)):
        items[slot] = (g[k], PC.blinding("g%d" % k))
        status[slot] = PC.OK
    out = run(keys, NTT, 9, items, 3)
    assert out["status"].tolist() == status
    held_to_the_chain(keys, NTT, 9, [items[s] for s in (0, 64, 1029)],
                      {k: (v[[0, 64, 1029]] if v is not None else None) for k, v in out.items()}, [PC.OK] * 3)
    rest = np.ones(1030, dtype=bool)
    rest[[0, 64, 1029]] = False
    for name in ("wire", "proofs", "instance", "num_unsatisfied"):
        assert not out[name][rest].any(), name


# ---- 4. edges ---------------------------------------------------------------------------------------------------------------------------
def test_edges(keys):
    g = PC.genuine(9, 2)
    one = [(g[0], PC.blinding("g0"))]
    held_to_the_chain(keys, NTT, 9, one, run(keys, NTT, 9, one, 1), [PC.OK])
    none = [(PC.bad_header(g[0]), PC.blinding("g0"))]
    held_to_the_chain(keys, NTT, 9, none, run(keys, NTT, 9, none, 1), [PC.DECODE])
    three = [(PC.bad_header(g[0]), PC.blinding("a")), (PC.at_the_bound(9), PC.blinding("b")), (PC.bad_key(g[1]), PC.blinding("c"))]
    held_to_the_chain(keys, NTT, 9, three, run(keys, NTT, 9, three, 2), [PC.DECODE, PC.NORM_BOUND, PC.DECODE])
    # an uncompressed wire mode; and none of the optional outputs
    two = [(g[0], PC.blinding("g0")), (PC.bad_key(g[1]), PC.blinding("x")), (g[1], PC.blinding("g1"))]
    out = run(keys, NTT, 9, two, 1, compressed=False)
    assert out["wire"].shape == (3, 384)
    held_to_the_chain(keys, NTT, 9, two, out, [PC.OK, PC.DECODE, PC.OK], compressed=False)
    assert [x == 1 for x in verdicts(keys, NTT, 9, out, compressed=False)] == [True, False, True]
    bare = run(keys, NTT, 9, two, 2, want=(False, False, False))
    held_to_the_chain(keys, NTT, 9, two, bare, [PC.OK, PC.DECODE, PC.OK])


def test_batch_zero_and_refused_arguments(keys):
    """batch = 0 is a no-op; with real handles: a circuit or parameter set that is not the handle's, an aggregate handle, a workspace
    one byte short of one proof in flight -> FRW_E_INVALID_ARG, and frw_pok_prove_workspace_bytes is 0 for the same mismatches"""
    import ctypes as C
    import torch
    import falcon_r1cs_amd as frw
    engine = keys.engine
    key, r1cs, _ = keys.get(NTT, 9)
    dev = torch.device("cuda:0")
    out = engine.pok_prove_from_bytes_dev(key, r1cs, NTT, 9, [], [], [], np.zeros((0, 2, 4), dtype=np.uint64), stream=_stream())
    assert out["wire"].shape == (0, 192) and out["status"].numel() == 0
    g = PC.genuine(9, 1)
    d_pkb, d_sgb, (d_blob, d_off), d_rs = _upload(9, [(g[0], PC.blinding("g0"))])
    need = engine.pok_prove_workspace_bytes(key, r1cs, NTT, 9, 1, 1)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    o = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(circuit=NTT, logn=9, r=r1cs, ws_bytes=need):
        return engine._lib.frw_pok_prove_from_bytes_dev(engine._ctx, key, r, circuit, logn, 1, p(d_pkb), p(d_sgb), 666, p(d_blob), p(d_off),
                                                        p(d_rs), 0, p(o), p(o), p(o), p(o), p(o), p(ws), ws_bytes, C.c_void_p(_stream()))
    assert call(circuit=DUAL) == -1 and call(circuit=SCHOOLBOOK) == -1 and call(logn=10) == -1
    assert call(ws_bytes=need - 1) == -1 and call(ws_bytes=0) == -1
    agg = engine.r1cs_load_aggregate([9, 9])
    try:
        assert call(r=agg) == -1
        assert engine.pok_prove_workspace_bytes(key, agg, NTT, 9, 1, 1) == 0
    finally:
        engine.r1cs_free(agg)
    for circuit, logn in ((DUAL, 9), (SCHOOLBOOK, 9), (NTT, 10)):
        assert engine.pok_prove_workspace_bytes(key, r1cs, circuit, logn, 1, 1) == 0
    torch.cuda.synchronize()
    assert not o.any()                                          # a refused call wrote nothing
    assert frw.ST_OK == 0


# ---- 5. the other circuits, and Falcon-1024 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("circuit,logn,shape", [(DUAL, 9, "aRa"), (SCHOOLBOOK, 9, "aR"), (NTT, 10, "aRa")])
def test_other_circuits_and_falcon_1024(keys, circuit, logn, shape):
    g = PC.genuine(logn, 2)
    items, status, k = [], [], 0
    for c in shape:
        if c == "a":
            items.append((g[k], PC.blinding("g%d/%d" % (k, logn))))
            status.append(PC.OK)
            k += 1
        else:
            items.append((PC.bad_header(g[0]), PC.blinding("refused")))
            status.append(PC.DECODE)
    out = run(keys, circuit, logn, items, 1)
    held_to_the_chain(keys, circuit, logn, items, out, status)
    assert [x == 1 for x in verdicts(keys, circuit, logn, out)] == [s == PC.OK for s in status]


# ---- 6. the host form -------------------------------------------------------------------------------------------------------------------
def test_host_form_equals_the_device_form(keys, mixed):
    import falcon_r1cs_amd as frw
    items, status, outs = mixed
    engine = keys.engine
    key, r1cs, _ = keys.get(NTT, 9)
    pkb, msgs, sgb = ([t[k] for t, _ in items] for k in range(3))
    rs = np.stack([r for _, r in items])
    host = engine.pok_prove_from_bytes(key, r1cs, NTT, 9, pkb, sgb, msgs, rs, strict=False)
    for name in ("wire", "proofs", "instance", "status", "num_unsatisfied"):
        assert np.array_equal(host[name], outs[2][name]), name
    # strict: FRW_E_RANGE, with every output complete
    lib = engine._lib
    import ctypes as C
    batch = len(items)
    blob = np.frombuffer(b"".join(msgs), dtype=np.uint8)
    off = np.zeros(batch + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    pk_arr, sg_arr = np.frombuffer(b"".join(pkb), dtype=np.uint8), np.frombuffer(b"".join(sgb), dtype=np.uint8)
    wire = np.full((batch, 192), 0xA5, dtype=np.uint8)
    proofs = np.full((batch, 48), 0xA5A5, dtype=np.uint64)
    inst = np.full((batch, 1025, 4), 0xA5A5, dtype=np.uint64)
    st = np.full(batch, -7, dtype=np.int32)
    uns = np.full(batch, 77, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.frw_pok_prove_from_bytes(engine._ctx, key, r1cs, NTT, 9, batch, p(pk_arr), p(sg_arr), 666, p(blob), p(off), p(rs), 0, p(wire), p(proofs),
                                      p(inst), p(st), p(uns), 1)
    assert rc == -5
    for name, got in (("wire", wire), ("proofs", proofs), ("instance", inst), ("status", st), ("num_unsatisfied", uns)):
        assert np.array_equal(got, outs[2][name]), name
    with pytest.raises(frw.FrwError):
        engine.pok_prove_from_bytes(key, r1cs, NTT, 9, pkb, sgb, msgs, rs)


def test_host_form_in_two_passes_equals_the_device_form(keys):
    """259 slots = one full pass of the host-buffer form (POK_PROVE_CHUNK = 256 in frw_capi.cpp) and three more.  Slots 0, 1 and 257
    genuine, every other one with a bad signature header: three proofs are made, one of them in the second pass.  The device form over the
    whole batch is the reference.  The genuine messages have different lengths, so the second pass's offsets have to be rebased."""
    engine = keys.engine
    key, r1cs, _ = keys.get(NTT, 9)
    g = PC.genuine(9, 3)
    assert len({len(t[1]) for t in g}) > 1
    batch, where = 259, (0, 1, 257)
    items = [(PC.bad_header(g[i % 3]), PC.blinding("refused")) for i in range(batch)]
    status = [PC.DECODE] * batch
    for slot, k in zip(where, range(3)):
        items[slot] = (g[k], PC.blinding("g%d" % k))
        status[slot] = PC.OK
    want = run(keys, NTT, 9, items, 3)
    assert want["status"].tolist() == status
    held_to_the_chain(keys, NTT, 9, [items[s] for s in where], {k: v[list(where)] for k, v in want.items()}, [PC.OK] * 3)
    pkb, msgs, sgb = ([t[k] for t, _ in items] for k in range(3))
    rs = np.stack([r for _, r in items])
    host = engine.pok_prove_from_bytes(key, r1cs, NTT, 9, pkb, sgb, msgs, rs, strict=False)
    for name in ("wire", "proofs", "instance", "status", "num_unsatisfied"):
        assert np.array_equal(host[name], want[name]), name
    rest = np.ones(batch, dtype=bool)
    rest[list(where)] = False
    for name in ("wire", "proofs", "instance", "num_unsatisfied"):
        assert not host[name][rest].any(), name
    assert all(host["wire"][s].any() for s in where)
