"""Re-randomising proofs on the device (frw_groth16_rerandomize_dev / _wire_dev, falcon-r1cs_amd/csrc/frw_rerand.hip) against the host
function (frw_groth16_rerandomize: the same formulas of frw_rerand.h in one thread, itself held to oracle/bls12_381.py by
tests/test_rerandomize_host.py), bit for bit -- an affine point has one representation.  Beside it: the oracle's fixed-base multiples
for the G1 points, the device verifier for the statements, the wire codec on the host for the wire form."""
import random

import numpy as np
import pytest

import frw_testlib as T
import rerandomize_cases as RC
from oracle import bls12_381 as E
from test_gpu_verify_dev import _dev, encode, key, proof_limbs, vectors

pytestmark = pytest.mark.gpu

R = E.R
N = 1025
DISTINCT = 8          # proofs made in Python integers (three scalar multiplications each); the batches tile them under fresh factors


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _np(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def case_env(oracle):
    import falcon_r1cs_amd as frw
    cs = RC.build(oracle)
    ver = frw.Groth16Verifier(cs.key.limbs(), device=0)
    yield cs, ver
    ver.close()


class Batch:
    """1,030 slots over DISTINCT proofs of DISTINCT statements of the n = 1025 key, with the exponents of A and C known"""

    def __init__(self, oracle):
        import falcon_r1cs_amd as frw
        self.k = key(oracle, N)
        self.ver = frw.Groth16Verifier(self.k.limbs(), device=0)
        rng = random.Random(99)
        rs = np.random.default_rng(99)
        vecs = vectors(N, rs)
        self.inst, self.proofs, self.a, self.c = [], [], [], []
        for i in range(DISTINCT):
            small, extra = vecs[i % len(vecs)]
            small = small.copy()
            small[1] = i                                           # (all statements different)
            acc = self.k.dot(small, extra)
            peek = random.Random()
            peek.setstate(rng.getstate())
            a, b = peek.randrange(1, R), peek.randrange(1, R)      # what Key.proof is about to draw
            p = self.k.proof(acc, rng)
            assert p[0] == E.mul(E.G1, a)
            self.a.append(a)
            self.c.append((a * b - self.k.alpha * self.k.beta - self.k.gamma * acc) * pow(self.k.delta, -1, R) % R)
            self.inst.append(encode(small, extra, True))
            self.proofs.append(proof_limbs(p))
        self.size = 1030
        self.which = np.arange(self.size) % DISTINCT
        self.all_proofs = np.stack([self.proofs[w] for w in self.which])
        self.factor_ints = [(rng.randrange(1, R), rng.randrange(1 << 256)) for _ in range(self.size)]
        self.all_factors = np.stack([T.ints_to_limbs(f) for f in self.factor_ints])
        self.want, self.want_status = self.ver.rerandomize(self.all_proofs, self.all_factors)
        assert not self.want_status.any()
        self.d_inst = _dev(np.stack(self.inst))


@pytest.fixture(scope="module")
def batch(oracle):
    b = Batch(oracle)
    yield b
    b.ver.close()


@pytest.mark.parametrize("vouched", [False, True])
def test_the_case_list_in_one_mixed_batch(case_env, vouched):
    import falcon_r1cs_amd as frw
    cs, ver = case_env
    flags = frw.VERIFY_POINTS_ARE_CHECKED if vouched else 0
    want, want_status = ver.rerandomize(cs.proofs(), cs.factors(), flags)
    out, status = ver.rerandomize_dev(_dev(cs.proofs()), _dev(cs.factors()), flags, stream=_stream())
    got, got_status = _np(out), status.cpu().numpy()
    assert got_status.tolist() == want_status.tolist()
    for i, c in enumerate(cs.cases):
        assert got[i].tolist() == want[i].tolist(), (c.name, vouched)
    RC.check(cs, got, got_status, vouched)                         # ... and so the oracle's


@pytest.mark.parametrize("size", [1, 2, 65, 1030])
def test_batch_sizes(oracle, batch, size):
    """a lone quad of lanes, a partial wavefront, more than one workgroup"""
    import torch
    b = batch
    d_proofs, d_factors = _dev(b.all_proofs[:size]), _dev(b.all_factors[:size])
    out, status = b.ver.rerandomize_dev(d_proofs, d_factors, stream=_stream())
    got = _np(out)
    assert status.cpu().tolist() == [0] * size
    assert got.tolist() == b.want[:size].tolist()
    # the G1 points from the exponents: A' = (a / r1) G1, C' = (c + r2 a) G1
    ea = [b.a[b.which[i]] * pow(b.factor_ints[i][0], -1, R) % R for i in range(size)]
    ec = [(b.c[b.which[i]] + b.factor_ints[i][1] * b.a[b.which[i]]) % R for i in range(size)]
    assert got[:, :12].tolist() == oracle.g1_fixed_base(T.ints_to_limbs(ea), threads=8).tolist()
    assert got[:, 36:].tolist() == oracle.g1_fixed_base(T.ints_to_limbs(ec), threads=8).tolist()
    # every slot verifies against its own statement and not against its neighbour's
    idx = torch.from_numpy(b.which[:size].copy()).to(out.device)
    assert b.ver.verify_full_dev(b.d_inst[idx], out, stream=_stream()).cpu().tolist() == [1] * size
    other = torch.from_numpy(((b.which[:size] + 1) % DISTINCT).copy()).to(out.device)
    assert b.ver.verify_full_dev(b.d_inst[other], out, stream=_stream()).cpu().tolist() == [0] * size


def test_a_slot_depends_on_itself_alone(batch):
    import falcon_r1cs_amd as frw
    import torch
    b = batch
    dev = torch.device("cuda:0")
    size = 65
    d_proofs, d_factors = _dev(b.all_proofs[:size]), _dev(b.all_factors[:size])
    alone, st = b.ver.rerandomize_dev(d_proofs[7:8], d_factors[7:8], stream=_stream())
    assert _np(alone)[0].tolist() == b.want[7].tolist() and st.cpu().tolist() == [0]
    # chunks of three: a workspace of exactly three proofs, and nothing written behind it
    buf, ws = T.guarded_workspace(b.ver.rerandomize_workspace_bytes(3), dev)
    out, st = b.ver.rerandomize_dev(d_proofs, d_factors, workspace=ws, stream=_stream())
    assert _np(out).tolist() == b.want[:size].tolist() and st.cpu().tolist() == [0] * size
    assert T.guard_intact(buf)
    # the whole batch in a workspace of exactly the reported size
    buf, ws = T.guarded_workspace(b.ver.rerandomize_workspace_bytes(size), dev)
    out, st = b.ver.rerandomize_dev(d_proofs, d_factors, workspace=ws, stream=_stream())
    assert _np(out).tolist() == b.want[:size].tolist() and T.guard_intact(buf)
    # in place
    same = d_proofs.clone()
    out, st = b.ver.rerandomize_dev(same, d_factors, out=same, stream=_stream())
    assert out.data_ptr() == same.data_ptr() and _np(same).tolist() == b.want[:size].tolist()
    # refusals that need a device: a workspace too small for one proof, a key without a device part
    with pytest.raises(frw.FrwError) as ei:
        b.ver.rerandomize_dev(d_proofs[:1], d_factors[:1], workspace=buf[:b.ver.rerandomize_workspace_bytes(1) - 1])
    assert ei.value.code == -1
    host = frw.Groth16Verifier(b.k.limbs())
    with pytest.raises(frw.FrwError) as ei:
        host.rerandomize_dev(d_proofs[:1], d_factors[:1], workspace=buf)
    assert ei.value.code == -1
    host.close()
    torch.cuda.synchronize()


@pytest.mark.parametrize("compressed", [True, False])
def test_wire_form(batch, compressed):
    import falcon_r1cs_amd as frw
    import torch
    b = batch
    dev = torch.device("cuda:0")
    size, per = 9, frw.proof_wire_bytes(compressed)
    wire_in, st = frw.proofs_to_wire(b.all_proofs[:size], compressed)
    assert not st.any()
    wire_in = wire_in.copy()
    wire_in[2, per - 1] |= 0xC0                                     # slot 2: both flag bits set -- malformed
    decoded, dst = frw.proofs_from_wire(wire_in, compressed)
    assert dst.tolist() == [0, 0, -1] + [0] * (size - 3)
    limbs, hst = b.ver.rerandomize(decoded, b.all_factors[:size])
    want, wst = frw.proofs_to_wire(limbs, compressed)
    assert not wst.any() and hst.tolist() == [0] * size             # (the host function sees three points at infinity in slot 2)
    d_wire = torch.from_numpy(wire_in.copy()).to(dev)
    d_factors = _dev(b.all_factors[:size])
    out, status = b.ver.rerandomize_wire_dev(d_wire, d_factors, compressed, stream=_stream())
    got = out.cpu().numpy()
    assert status.cpu().tolist() == [0, 0, -1] + [0] * (size - 3)
    assert not got[2].any()                                         # zero BYTES, not three encoded points at infinity
    for i in range(size):
        if i != 2:
            assert got[i].tolist() == want[i].tolist(), i
            assert got[i].tolist() == frw.proofs_to_wire(b.want[i:i + 1], compressed)[0][0].tolist()
    # chunks of two with an exact workspace, then in place
    mode = frw.engine.WIRE_COMPRESSED if compressed else frw.engine.WIRE_UNCOMPRESSED
    buf, ws = T.guarded_workspace(b.ver.rerandomize_workspace_bytes(2, mode), dev)
    out2, status2 = b.ver.rerandomize_wire_dev(d_wire, d_factors, compressed, workspace=ws, stream=_stream())
    assert torch.equal(out2, out) and torch.equal(status2, status) and T.guard_intact(buf)
    same = d_wire.clone().reshape(size, per)
    out3, status3 = b.ver.rerandomize_wire_dev(same, d_factors, compressed, out=same, stream=_stream())
    assert torch.equal(same, out) and torch.equal(status3, status)


def test_graph_capture_on_one_stream(batch):
    import torch
    b = batch
    size = 5
    d_proofs = _dev(b.all_proofs[:size])
    d_factors = _dev(b.all_factors[:size])
    second = b.all_factors[size:2 * size]
    want2, _ = b.ver.rerandomize(b.all_proofs[:size], second)
    out = torch.zeros((size, 48), dtype=torch.int64, device=d_proofs.device)
    ws = torch.empty(b.ver.rerandomize_workspace_bytes(size), dtype=torch.uint8, device=d_proofs.device)
    holder = {}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            _, holder["status"] = b.ver.rerandomize_dev(d_proofs, d_factors, out=out, workspace=ws, stream=s.cuda_stream)
        graph.replay()
        s.synchronize()
        assert _np(out).tolist() == b.want[:size].tolist() and holder["status"].cpu().tolist() == [0] * size
        d_factors.copy_(_dev(second))
        graph.replay()
        s.synchronize()
        assert _np(out).tolist() == want2.tolist()
    torch.cuda.current_stream().wait_stream(s)


def test_falcon_512_prove_rerandomize_verify(engine):
    """pok_prove_from_bytes_dev -> rerandomize_wire_dev -> verify_statements_wire_dev: three proofs of real signatures"""
    import falcon_r1cs_amd as frw
    import pok_prove_cases as PC
    import torch
    logn = 9
    rng = random.Random(31)
    triples = PC.genuine(logn, 3)
    key_, vk = engine.groth16_setup(frw.CIRCUIT_NTT, logn, *(rng.randrange(2, R) for _ in range(5)))
    r1cs = engine.r1cs_load(frw.CIRCUIT_NTT, logn)
    ver = frw.Groth16Verifier.from_wire(frw.vk_to_wire(vk), device=0)
    rs = np.stack([PC.blinding(i) for i in range(3)])
    pkb, msgs, sgb = ([t[k] for t in triples] for k in range(3))
    out = engine.pok_prove_from_bytes_dev(key_, r1cs, frw.CIRCUIT_NTT, logn, pkb, sgb, msgs, rs, in_flight=3, want_proofs=False,
                                          want_instance=False, stream=_stream())
    assert out["status"].tolist() == [0, 0, 0]
    d_factors = _dev(np.stack([T.ints_to_limbs([rng.randrange(1, R), rng.randrange(1, R)]) for _ in range(3)]))
    fresh, status = ver.rerandomize_wire_dev(out["wire"].reshape(-1), d_factors, stream=_stream())
    assert status.cpu().tolist() == [0, 0, 0]
    old, new = out["wire"].cpu().numpy().reshape(3, 192), fresh.cpu().numpy()
    for i in range(3):
        assert all(old[i, lo:hi].tolist() != new[i, lo:hi].tolist() for lo, hi in ((0, 48), (48, 144), (144, 192)))
    nonces = [s[1:1 + frw.NONCE_LEN] for s in sgb]
    st, verdict = ver.verify_statements_wire_dev(engine, logn, pkb, nonces, msgs, fresh)
    assert st.tolist() == [0, 0, 0] and verdict.tolist() == [1, 1, 1]
    st, verdict = ver.verify_statements_wire_dev(engine, logn, pkb, nonces, [msgs[1], msgs[2], msgs[0]], fresh)
    assert verdict.tolist() == [0, 0, 0]
    ver.close()
    engine.r1cs_free(r1cs)
    engine.groth16_pk_free(key_)
