"""Drawing Groth16's blinding and re-randomising factors on the device (falcon-r1cs_amd/csrc/frw_drbg.hip: frw_fr_draw_dev and the three
*_seeded_dev calls) against hashlib and Python integers (tests/drbg_ref.py), bit for bit: the draw itself and its counter; the seeded
prover on the cubic system of examples/custom_r1cs.py against the un-seeded prover given the reference's factors; a captured seeded
prover (Falcon-512, the existing capture test's shape) replayed three times with the host out of the loop, fresh every time; the seeded
re-randomisers against the un-seeded ones, and a captured one against the host function."""
import importlib.util
import os
import random

import numpy as np
import pytest

import drbg_ref as D
import frw_testlib as T
import rerandomize_cases as RC
from oracle import bls12_381 as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = (1 << 64) - 1
SEED2 = bytes(random.Random(1600).getrandbits(8) for _ in range(32))
POINTS = ((0, 12), (12, 36), (36, 48))              # A | B | C in a proof's 48 words


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _seed(seed):
    import torch
    return torch.from_numpy(np.frombuffer(seed, dtype=np.uint8).copy()).to("cuda:0")


def _counter(c):
    import torch
    return torch.tensor([c - (1 << 64) if c >> 63 else c], dtype=torch.int64, device="cuda:0")


def _read(d_counter):
    return int(d_counter.cpu()[0]) & MASK


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).to("cuda:0")


def _np(t):
    return t.cpu().numpy().view(np.uint64)


def _no_point_in_common(proofs):
    """proofs: uint64[k, 48] -- no two of them share A, B or C"""
    return all(len({p[lo:hi].tobytes() for p in proofs}) == len(proofs) for lo, hi in POINTS)


# ---- 1. the draw --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", [D.BLINDING, D.RERANDOMIZE])
def test_the_draw_against_hashlib(tag):
    """a lone lane, a wavefront less one, exactly one, one more (two workgroups), several and a partial last one"""
    import torch
    import falcon_r1cs_amd as frw
    d_seed = _seed(D.SEED)
    for count, start in ((1, 0), (63, (1 << 32) - 1), (64, (1 << 64) - 1), (65, 0), (257, (1 << 32) - 1), (1000, (1 << 64) - 1)):
        d_counter = _counter(start)
        buf, out = T.guarded_workspace(count * 32, torch.device("cuda:0"))
        got = frw.fr_draw_dev(d_seed, d_counter, tag, count, out=out, stream=_stream())
        assert got.data_ptr() == out.data_ptr()
        words = out.cpu().numpy().view(np.uint64).reshape(count, 4)
        assert words.tolist() == D.draw(D.SEED, start, tag, count).tolist(), (count, start)
        assert words.tolist() == frw.fr_draw(D.SEED, start, tag, count).tolist()
        assert T.guard_intact(buf), count
        assert _read(d_counter) == (start + 1) & MASK                            # 2^64 - 1 reads back as 0
    assert _seed(D.SEED).cpu().numpy().tobytes() == D.SEED == d_seed.cpu().numpy().tobytes()


def test_the_counter_steps_once_a_call_and_not_for_an_empty_one():
    import torch
    import falcon_r1cs_amd as frw
    d_seed = _seed(SEED2)
    for c in (0, (1 << 32) - 1, (1 << 64) - 1):
        d_counter = _counter(c)
        first = frw.fr_draw_dev(d_seed, d_counter, 7, 65, stream=_stream())
        second = frw.fr_draw_dev(d_seed, d_counter, 7, 65, stream=_stream())
        assert _np(first).tolist() == D.draw(SEED2, c, 7, 65).tolist()
        assert _np(second).tolist() == D.draw(SEED2, (c + 1) & MASK, 7, 65).tolist()
        assert _read(d_counter) == (c + 2) & MASK
    out = torch.full((4, 4), 0x5A5A, dtype=torch.int64, device="cuda:0")
    d_counter = _counter(41)
    frw.fr_draw_dev(d_seed, d_counter, 1, 0, out=out, stream=_stream())
    torch.cuda.synchronize()
    assert _read(d_counter) == 41 and bool((out == 0x5A5A).all())
    with pytest.raises(frw.FrwError) as ei:
        frw.fr_draw_dev(d_seed, d_counter, 256, 4, out=out, stream=_stream())
    assert ei.value.code == -1 and _read(d_counter) == 41 and bool((out == 0x5A5A).all())


def test_tag_separation():
    import falcon_r1cs_amd as frw
    d_seed = _seed(D.SEED)
    a = _np(frw.fr_draw_dev(d_seed, _counter(9), D.BLINDING, 257, stream=_stream()))
    b = _np(frw.fr_draw_dev(d_seed, _counter(9), D.RERANDOMIZE, 257, stream=_stream()))
    assert a.tolist() == D.draw(D.SEED, 9, 1, 257).tolist() and b.tolist() == D.draw(D.SEED, 9, 2, 257).tolist()
    assert not {r.tobytes() for r in a} & {r.tobytes() for r in b}
    assert len({r.tobytes() for r in a}) == 257


# ---- 2. the seeded prover on the cubic system -----------------------------------------------------------------------------------------------
def _cubic_example():
    spec = importlib.util.spec_from_file_location("custom_r1cs_example", os.path.join(ROOT, "examples", "custom_r1cs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def cubic(engine, tmp_path_factory):
    """x^3 + x + 5 = y: I = 2, W = 3, C = 3, the 2^3 domain; five statements"""
    import torch
    import falcon_r1cs_amd as frw
    ex = _cubic_example()
    ONE, Y, X, X2, X3 = range(5)
    a = [[(1, X)], [(1, X2)], [(1, X3), (1, X), (5, ONE)]]
    b = [[(1, X)], [(1, X)], [(1, ONE)]]
    c = [[(1, X2)], [(1, X3)], [(1, Y)]]
    path = str(tmp_path_factory.mktemp("cubic") / "cubic.r1cs")
    ex.write_r1cs(path, 2, 3, (a, b, c))
    r1cs = engine.r1cs_load_file(path)
    info = engine.r1cs_info(r1cs)
    assert (info.num_instance, info.num_witness, info.num_constraints, info.log_domain_size) == (2, 3, 3, 3)
    rng = random.Random(513)
    key, vk = engine.groth16_setup_r1cs(r1cs, *(rng.randrange(2, D.R) for _ in range(5)))
    xs = [3, 4, D.R - 2, 1 << 200, 0]
    wit = torch.cat([ex.montgomery([x, x * x, x ** 3]) for x in xs]).to("cuda:0")
    inst = torch.cat([ex.montgomery([1, x ** 3 + x + 5]) for x in xs]).to("cuda:0")
    ver = frw.Groth16Verifier(vk)
    yield key, r1cs, wit, inst, ver
    ver.close()
    engine.groth16_pk_free(key)
    engine.r1cs_free(r1cs)


@pytest.mark.parametrize("batch", [1, 5])
def test_the_seeded_prover_on_the_cubic_system(engine, cubic, batch):
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    key, r1cs, wit, inst, ver = cubic
    wit, inst = wit[:batch].contiguous(), inst[:batch].contiguous()
    c = (1 << 32) - 1 + batch
    d_seed, d_counter = _seed(SEED2), _counter(c)
    ws_bytes = engine.groth16_workspace_bytes(key, r1cs, batch)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    d_rs = torch.zeros((batch, 2, 4), dtype=torch.int64, device=dev)
    got = torch.zeros((batch, 48), dtype=torch.int64, device=dev)
    bad = torch.full((batch,), -1, dtype=torch.int32, device=dev)
    engine.groth16_prove_seeded_dev(key, r1cs, batch, wit, inst, d_seed, d_counter, d_rs, got, ws, ws_bytes, bad, _stream())
    torch.cuda.synchronize()
    want_rs = D.factors(SEED2, c, D.BLINDING, batch)
    assert _np(d_rs).tolist() == want_rs.tolist()                               # slot i: elements 2 i and 2 i + 1
    assert _read(d_counter) == c + 1 and bad.tolist() == [0] * batch
    want = torch.zeros((batch, 48), dtype=torch.int64, device=dev)
    engine.groth16_prove_rs_dev(key, r1cs, batch, wit, inst, _dev(want_rs), want, ws, ws_bytes, None, _stream())
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert ver.verify(_np(inst), _np(got)).tolist() == [1] * batch
    if batch == 1:
        return
    # a workspace of two proofs for five (the chunk loop): the same factors from the same counter, the same bytes, ONE step of the counter
    ws2_bytes = engine.groth16_workspace_bytes(key, r1cs, 2)
    buf, ws2 = T.guarded_workspace(ws2_bytes, dev)
    d_counter2 = _counter(c)
    d_rs2 = torch.zeros_like(d_rs)
    got2 = torch.zeros_like(got)
    engine.groth16_prove_seeded_dev(key, r1cs, batch, wit, inst, d_seed, d_counter2, d_rs2, got2, ws2, ws2_bytes, None, _stream())
    torch.cuda.synchronize()
    assert torch.equal(got2, want) and torch.equal(d_rs2, d_rs) and _read(d_counter2) == c + 1 and T.guard_intact(buf)
    # one byte short of one proof's workspace: refused, nothing drawn, the counter where it was
    d_rs2.fill_(0x77)
    with pytest.raises(frw.FrwError) as ei:
        engine.groth16_prove_seeded_dev(key, r1cs, batch, wit, inst, d_seed, d_counter2, d_rs2, got2, ws2,
                                        engine.groth16_workspace_bytes(key, r1cs, 1) - 1, None, _stream())
    torch.cuda.synchronize()
    assert ei.value.code == -1 and _read(d_counter2) == c + 1 and bool((d_rs2 == 0x77).all())


# ---- 3. captured and replayed: fresh every time ---------------------------------------------------------------------------------------------
def test_a_captured_seeded_prover_is_fresh_on_every_replay(engine):
    """the shape of tests/test_gpu_groth16.py's capture test: Falcon-512, batch 3, a side stream, thread-local capture errors"""
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    logn, batch = 9, 3
    L = frw.layout(logn)
    rng = random.Random(811)
    key, vk = engine.groth16_setup(0, logn, *(rng.randrange(2, E.R) for _ in range(5)))
    r1cs = engine.r1cs_load(0, logn)
    try:
        sig, pk_, hm = frw.synth_triples(logn, batch, seed=99)
        dd = [torch.from_numpy(a.view(np.int16)).to(dev) for a in (sig, pk_, hm)]
        wit = torch.empty((batch, L.num_witness, 4), dtype=torch.int64, device=dev)
        inst = torch.empty((batch, L.num_instance, 4), dtype=torch.int64, device=dev)
        st = torch.empty(batch, dtype=torch.int32, device=dev)
        engine.witness_ntt_verify_dev(logn, batch, dd[0], dd[1], dd[2], wit, inst, st, 1, _stream())
        torch.cuda.synchronize()
        ws_bytes = engine.groth16_workspace_bytes(key, r1cs, batch)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        c = (1 << 64) - 2                                                        # the replays cross the wrap: c, c + 1 = 2^64 - 1, 0
        d_seed, d_counter = _seed(D.SEED), _counter(c)
        d_rs = torch.zeros((batch, 2, 4), dtype=torch.int64, device=dev)
        got = torch.zeros((batch, 48), dtype=torch.int64, device=dev)
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            engine.groth16_prove_seeded_dev(key, r1cs, batch, wit, inst, d_seed, d_counter, d_rs, got, ws, ws_bytes, None, side.cuda_stream)   # warm the capture stream
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
                engine.groth16_prove_seeded_dev(key, r1cs, batch, wit, inst, d_seed, d_counter, d_rs, got, ws, ws_bytes, None,
                                                torch.cuda.current_stream().cuda_stream)
        assert _read(d_counter) == c + 1                                         # the warm-up's step; capturing ran nothing
        d_counter.copy_(_counter(c))
        torch.cuda.synchronize()
        outs, used = [], []
        for k in range(3):                                                       # nothing but replays: the host is out of the loop
            graph.replay()
            outs.append(got.clone())
            used.append(d_rs.clone())
        torch.cuda.synchronize()
        assert _read(d_counter) == (c + 3) & MASK
        for k in range(3):
            want_rs = D.factors(D.SEED, (c + k) & MASK, D.BLINDING, batch)
            assert _np(used[k]).tolist() == want_rs.tolist(), "replay %d" % k
            want = torch.zeros((batch, 48), dtype=torch.int64, device=dev)
            engine.groth16_prove_rs_dev(key, r1cs, batch, wit, inst, _dev(want_rs), want, ws, ws_bytes, None, _stream())
            torch.cuda.synchronize()
            assert torch.equal(outs[k], want), "replay %d" % k
        ver = frw.Groth16Verifier(vk)
        for i in range(batch):
            assert _no_point_in_common([_np(o)[i] for o in outs]), i
        for k in range(3):
            assert ver.verify(_np(inst), _np(outs[k])).tolist() == [1] * batch, "replay %d" % k
        ver.close()
    finally:
        engine.r1cs_free(r1cs)
        engine.groth16_pk_free(key)


# ---- 4. the seeded re-randomisers ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case_env(oracle):
    import falcon_r1cs_amd as frw
    cs = RC.build(oracle)
    ver = frw.Groth16Verifier(cs.key.limbs(), device=0)
    yield cs, ver
    ver.close()


def test_the_seeded_rerandomiser_is_the_unseeded_one_with_the_reference_factors(case_env):
    """the whole case list (malformed proofs among it: the statuses are the wrapped call's), in place, and two proofs in flight for five"""
    import torch
    import falcon_r1cs_amd as frw
    cs, ver = case_env
    dev = torch.device("cuda:0")
    proofs = cs.proofs()
    n, c = len(proofs), 1 << 32
    d_seed, d_counter = _seed(SEED2), _counter(c)
    d_proofs = _dev(proofs)
    out, status, d_factors = ver.rerandomize_seeded_dev(d_proofs, d_seed, d_counter, stream=_stream())
    want_f = D.factors(SEED2, c, D.RERANDOMIZE, n)
    assert _np(d_factors).tolist() == want_f.tolist() and _read(d_counter) == c + 1
    want, want_status = ver.rerandomize_dev(d_proofs, _dev(want_f), stream=_stream())
    assert torch.equal(out, want) and torch.equal(status, want_status)
    assert 0 in status.tolist() and -1 in status.tolist()
    host, host_status = ver.rerandomize(proofs, want_f)
    assert _np(out).tolist() == host.tolist() and status.cpu().tolist() == host_status.tolist()
    # in place, the next counter
    same = d_proofs.clone()
    out2, status2, f2 = ver.rerandomize_seeded_dev(same, d_seed, d_counter, out=same, stream=_stream())
    assert out2.data_ptr() == same.data_ptr() and _read(d_counter) == c + 2
    want_f2 = D.factors(SEED2, c + 1, D.RERANDOMIZE, n)
    want2, want_status2 = ver.rerandomize_dev(d_proofs, _dev(want_f2), stream=_stream())
    assert _np(f2).tolist() == want_f2.tolist() and torch.equal(same, want2) and torch.equal(status2, want_status2)
    # five proofs through a workspace of exactly two: the factors of ONE draw, one step of the counter
    buf, ws = T.guarded_workspace(ver.rerandomize_workspace_bytes(2), dev)
    d_counter3 = _counter(c)
    out3, status3, f3 = ver.rerandomize_seeded_dev(d_proofs[:5], d_seed, d_counter3, workspace=ws, stream=_stream())
    assert torch.equal(f3, d_factors[:5]) and torch.equal(out3, want[:5]) and torch.equal(status3, want_status[:5])
    assert _read(d_counter3) == c + 1 and T.guard_intact(buf)
    # refused (a workspace too small for one proof; a bad flag): nothing drawn, the counter where it was
    f3.fill_(0x77)
    for kw in (dict(workspace=buf[:ver.rerandomize_workspace_bytes(1) - 1]), dict(flags=4)):
        with pytest.raises(frw.FrwError) as ei:
            ver.rerandomize_seeded_dev(d_proofs[:5], d_seed, d_counter3, d_factors=f3, stream=_stream(), **kw)
        assert ei.value.code == -1
    torch.cuda.synchronize()
    assert _read(d_counter3) == c + 1 and bool((f3 == 0x77).all())


@pytest.mark.parametrize("compressed", [True, False])
def test_the_seeded_wire_rerandomiser(case_env, compressed):
    import torch
    import falcon_r1cs_amd as frw
    cs, ver = case_env
    dev = torch.device("cuda:0")
    good = [i for i, k in enumerate(cs.cases) if k.status == 0 and k.status_vouched == 0][:9]
    wire_in, st = frw.proofs_to_wire(cs.proofs()[good], compressed)
    assert not st.any()
    wire_in = wire_in.copy()
    per = frw.proof_wire_bytes(compressed)
    wire_in[2, per - 1] |= 0xC0                                                  # slot 2: both flag bits set -- malformed
    n, c = len(good), (1 << 64) - 1
    d_wire = torch.from_numpy(wire_in).to(dev)
    d_seed, d_counter = _seed(D.SEED), _counter(c)
    out, status, d_factors = ver.rerandomize_wire_seeded_dev(d_wire, d_seed, d_counter, compressed=compressed, stream=_stream())
    want_f = D.factors(D.SEED, c, D.RERANDOMIZE, n)
    assert _np(d_factors).tolist() == want_f.tolist() and _read(d_counter) == 0
    want, want_status = ver.rerandomize_wire_dev(d_wire, _dev(want_f), compressed, stream=_stream())
    assert torch.equal(out, want) and torch.equal(status, want_status)
    assert status.cpu().tolist() == [0, 0, -1] + [0] * (n - 3)
    # two in flight with an exact workspace, then in place
    mode = frw.engine.WIRE_COMPRESSED if compressed else frw.engine.WIRE_UNCOMPRESSED
    buf, ws = T.guarded_workspace(ver.rerandomize_workspace_bytes(2, mode), dev)
    d_counter2 = _counter(c)
    out2, status2, f2 = ver.rerandomize_wire_seeded_dev(d_wire, d_seed, d_counter2, compressed=compressed, workspace=ws, stream=_stream())
    assert torch.equal(out2, want) and torch.equal(status2, want_status) and torch.equal(f2, d_factors)
    assert _read(d_counter2) == 0 and T.guard_intact(buf)
    same = d_wire.clone().reshape(n, per)
    d_counter3 = _counter(c)
    out3, status3, _ = ver.rerandomize_wire_seeded_dev(same, d_seed, d_counter3, compressed=compressed, out=same, stream=_stream())
    assert torch.equal(same, want) and torch.equal(status3, want_status)


def test_a_captured_seeded_rerandomiser_is_fresh_on_every_replay(case_env):
    """one stream, five copies of a proof that verifies: three replays are the host function with the factors of c, c + 1, c + 2"""
    import torch
    import falcon_r1cs_amd as frw
    cs, ver = case_env
    size, c = 5, 77
    valid = cs.cases[0].proof
    proofs = np.stack([valid] * size)
    d_proofs = _dev(proofs)
    d_seed, d_counter = _seed(SEED2), _counter(c)
    d_factors = torch.zeros((size, 2, 4), dtype=torch.int64, device=d_proofs.device)
    out = torch.zeros((size, 48), dtype=torch.int64, device=d_proofs.device)
    ws = torch.empty(ver.rerandomize_workspace_bytes(size), dtype=torch.uint8, device=d_proofs.device)
    holder = {}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    outs = []
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            _, holder["status"], _ = ver.rerandomize_seeded_dev(d_proofs, d_seed, d_counter, d_factors=d_factors, out=out, workspace=ws,
                                                                stream=s.cuda_stream)
        for k in range(3):
            graph.replay()
            outs.append(out.clone())
        s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    assert _read(d_counter) == c + 3 and holder["status"].cpu().tolist() == [0] * size
    inst = T.ints_to_limbs([1] + cs.statement)[None].repeat(size, axis=0)
    for k in range(3):
        want, want_status = ver.rerandomize(proofs, D.factors(SEED2, c + k, D.RERANDOMIZE, size))
        assert not want_status.any() and _np(outs[k]).tolist() == want.tolist(), "replay %d" % k
        assert ver.verify(inst, _np(outs[k]), frw.ENC_CANONICAL).tolist() == [1] * size
    assert _no_point_in_common([valid] + [p for o in outs for p in _np(o)])
