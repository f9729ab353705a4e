"""ark-serialize's wire format on the device (frw_wire.hip): the device codec against the host's byte for byte, verification from wire
bytes (frw_groth16_verify_wire_dev) against frw_groth16_verify_full_dev on the decoded limbs verdict for verdict, keys loaded from bytes
with gamma_abc_g1 decoded on the device.  The host codec is checked against tests/wire_ref.py in test_wire_codec.py; statements are made
"in the exponent" with test_gpu_verify_dev.py's key and test_gpu_verify_full.py's mixed batch."""
import ctypes as C
import random

import numpy as np
import pytest

import frw_testlib as T
import wire_ref as W
from oracle import bls12_381 as E
from test_gpu_verify_dev import R, _dev, encode, key, proof_limbs
from test_gpu_verify_full import _accepted_and_refused, _batch, _mixed_cases
from test_wire_codec import g2_points_whose_y_squared_has_no_u_part, malformed_cases

pytestmark = pytest.mark.gpu
Q = E.Q
_FALCON = {}


def _falcon(engine, logn, batch=3):
    """`batch` real Falcon proofs: (instance vectors, proofs) as device tensors and the verifying key, made once per size"""
    import torch
    import falcon_r1cs_amd as frw
    if logn in _FALCON:
        return _FALCON[logn]
    dev = torch.device("cuda:0")
    L = frw.layout(logn)
    rng = random.Random(800 + logn)
    pk, vk = engine.groth16_setup(0, logn, *(rng.randrange(2, R) for _ in range(5)))
    r1cs = engine.r1cs_load(0, logn)
    try:
        sig, pk_, hm = frw.synth_triples(logn, batch, seed=43 + logn)
        dd = [torch.from_numpy(a.view(np.int16)).to(dev) for a in (sig, pk_, hm)]
        wit = torch.empty((batch, L.num_witness, 4), dtype=torch.int64, device=dev)
        inst = torch.empty((batch, L.num_instance, 4), dtype=torch.int64, device=dev)
        st = torch.empty(batch, dtype=torch.int32, device=dev)
        s0 = torch.cuda.current_stream().cuda_stream
        engine.witness_ntt_verify_dev(logn, batch, dd[0], dd[1], dd[2], wit, inst, st, frw.ENC_MONTGOMERY, s0)
        rs = np.array([T.ints_to_limbs([rng.randrange(R), rng.randrange(R)]) for _ in range(batch)])
        ws_bytes = engine.groth16_workspace_bytes(pk, r1cs, batch)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        proofs = torch.empty((batch, 48), dtype=torch.int64, device=dev)
        engine.groth16_prove_dev(pk, r1cs, batch, wit, inst, rs, proofs, ws, ws_bytes, None, s0)
        torch.cuda.synchronize()
    finally:
        engine.r1cs_free(r1cs)
        engine.groth16_pk_free(pk)
    _FALCON[logn] = (inst, proofs, vk)
    return _FALCON[logn]


def _g2neg(p):
    return (p[0], ((-p[1][0]) % Q, (-p[1][1]) % Q))


def _synthetic(oracle, count):
    """`count` proofs' limbs from multiples of the generators, their negatives and infinity -- and, for B, curve points whose y^2 lies
    in Fq (the Fq2 root's a1 = 0 branch)"""
    rng = random.Random(1234)
    ks = T.ints_to_limbs([rng.randrange(1, R) for _ in range(200)])
    g1 = oracle.g1_fixed_base(ks, threads=8)
    g1 = np.concatenate([g1, np.zeros((1, 12), dtype=np.uint64), np.stack([np.array(E.to_limbs(E.neg(E.from_limbs(p))), dtype=np.uint64) for p in g1[:40]])])
    g2p = [E.g2_mul(E.G2, rng.randrange(1, R)) for _ in range(24)]
    g2 = np.stack([np.array(E.g2_to_limbs(p), dtype=np.uint64) for p in g2p + [_g2neg(p) for p in g2p] + [None] + g2_points_whose_y_squared_has_no_u_part()[:12]])
    out = np.zeros((count, 48), dtype=np.uint64)
    for i in range(count):
        out[i, :12] = g1[i % len(g1)]
        out[i, 12:36] = g2[(5 * i + 1) % len(g2)]
        out[i, 36:] = g1[(7 * i + 3) % len(g1)]
    return out


@pytest.mark.parametrize("compressed", [True, False])
def test_device_codec_equals_the_hosts_on_a_mixed_batch(engine, oracle, compressed):
    import torch
    import falcon_r1cs_amd as frw
    count = 1100
    limbs = _synthetic(oracle, count)
    real = _falcon(engine, 9)[1].cpu().numpy().view(np.uint64)
    for j in range(real.shape[0]):                                             # real prover output among them
        limbs[11 + 100 * j] = real[j]
    # encoding: a coordinate >= q here and there
    enc_in = limbs.copy()
    refused = list(range(5, count, 97))
    for n, i in enumerate(refused):
        first = (0, 6, 12, 18, 24, 30, 36, 42)[n % 8]
        v = int.from_bytes(enc_in[i, first:first + 6].tobytes(), "little") + Q
        if v >> 384:
            v = Q
        enc_in[i, first:first + 6] = np.frombuffer(v.to_bytes(48, "little"), dtype=np.uint64)
    want, want_st = frw.proofs_to_wire(enc_in, compressed)
    assert [i for i in range(count) if want_st[i]] == refused
    got, got_st = frw.proofs_to_wire_dev(_dev(enc_in), compressed)
    assert got.is_cuda and got.shape == want.shape
    assert np.array_equal(got_st.cpu().numpy(), want_st)
    assert np.array_equal(got.cpu().numpy(), want)
    # decoding: every malformed case interleaved with the valid ones
    wire, st = frw.proofs_to_wire(limbs, compressed)
    assert not st.any()
    good = W.proof_encode((E.G1, E.G2, E.mul(E.G1, 9)), compressed)
    bad = malformed_cases(compressed, good)
    where = {}
    for n, (name, b) in enumerate(bad.items()):
        for i in (3 + 41 * n, 700 + 13 * n):
            wire[i] = np.frombuffer(b, dtype=np.uint8)
            where[i] = name
    want, want_st = frw.proofs_from_wire(wire, compressed)
    assert [i for i in range(count) if want_st[i]] == sorted(where)
    ok = np.array([i not in where for i in range(count)])
    assert np.array_equal(want[ok], limbs[ok]) and not want[~ok].any()
    dev = torch.device("cuda:0")
    for shift in (0, 1):                                                      # (an odd address too)
        buf = torch.zeros(wire.size + 16, dtype=torch.uint8, device=dev)
        d_wire = buf[shift:shift + wire.size]
        d_wire.copy_(torch.from_numpy(wire.reshape(-1)).to(dev))
        got, got_st = frw.proofs_from_wire_dev(d_wire, compressed)
        torch.cuda.synchronize()
        got_st = got_st.cpu().numpy()
        for i in range(count):
            assert got_st[i] == want_st[i], (i, where.get(i))
        assert np.array_equal(got.cpu().numpy().view(np.uint64), want)


@pytest.mark.parametrize("compressed", [True, False])
def test_verdicts_from_wire_bytes_equal_verify_full_dev_on_the_decoded_limbs(oracle, compressed):
    import torch
    import falcon_r1cs_amd as frw
    n = 1025
    k = key(oracle, n)
    cases = _mixed_cases(k, n, True, random.Random(11), np.random.default_rng(11))
    inst, proofs = _batch(k, n, 40, random.Random(5), np.random.default_rng(5), distinct=8)
    inst = np.concatenate([np.stack([c[0] for c in cases]), inst])
    limbs = np.concatenate([np.stack([c[1] for c in cases]), proofs])
    wire, enc_st = frw.proofs_to_wire(limbs, compressed)                      # (an alias x + q is refused here: zero bytes)
    good = W.proof_encode((E.G1, E.G2, E.mul(E.G1, 9)), compressed)
    undecodable = {}
    for j, (name, b) in enumerate(malformed_cases(compressed, good).items()):
        if j < 6:
            undecodable[len(cases) + 2 + 5 * j] = name
            wire[len(cases) + 2 + 5 * j] = np.frombuffer(b, dtype=np.uint8)
    decoded, dec_st = frw.proofs_from_wire(wire, compressed)
    assert all(dec_st[i] == -1 for i in undecodable)
    ver = frw.Groth16Verifier(k.limbs(), device=0)
    dev = torch.device("cuda:0")
    d_inst, d_wire = _dev(inst), torch.from_numpy(wire).to(dev)
    count = wire.shape[0]
    passed = torch.full((1,), 7, dtype=torch.int32, device=dev)
    seed = np.array([9, 8, 7, 6], dtype=np.uint64)
    for flags in (0, frw.VERIFY_POINTS_ARE_CHECKED):
        ref = ver.verify_full_dev(d_inst, _dev(decoded), flags=flags).cpu().tolist()
        want = [-1 if dec_st[i] else ref[i] for i in range(count)]
        if flags == 0:
            # the kinds the batch must hold: accepted, tampered, decodable but outside the subgroup, undecodable
            assert want[:3] == [1, 1, 0] and 1 in want[len(cases):]
            stray = len(cases) - 5                                             # _mixed_cases: A outside G1
            assert dec_st[stray] == 0 and want[stray] == -1
            assert all(want[i] == -1 for i in undecodable)
        for batched in (False, True):
            bflags = flags | (frw.VERIFY_BATCHED if batched else 0)
            full = ver.wire_workspace_bytes(count, bflags, compressed)
            small = ver.wire_workspace_bytes(7, bflags, compressed)
            assert 0 < small < full and full == ver.full_workspace_bytes(count, bflags) + 384 * count + ((4 * count + 15) & ~15)
            for size in (full, small):                                        # the whole batch at once, and in chunks of 7
                ws = torch.empty(size, dtype=torch.uint8, device=dev)
                got = ver.verify_wire_dev(d_inst, d_wire, compressed, flags=flags, batched=batched, seed=seed, workspace=ws, batch_passed=passed)
                assert got.cpu().tolist() == want, (flags, batched, size)
                if batched:
                    same = ver.verify_full_dev(d_inst, _dev(decoded), flags=flags, batched=True, seed=seed).cpu().tolist()
                    assert [-1 if dec_st[i] else same[i] for i in range(count)] == want
    # refusals: a bad mode, a small or misaligned workspace, a batched request without a seed
    lib = frw.load_library()
    out = torch.empty(count, dtype=torch.int32, device=dev)
    ws = torch.empty(ver.wire_workspace_bytes(count, 0, compressed), dtype=torch.uint8, device=dev)
    mode = 0 if compressed else 1
    args = lambda ptr, size, mode=mode, flags=0: (ver._h, count, C.c_void_p(d_inst.data_ptr()), frw.ENC_MONTGOMERY, C.c_void_p(d_wire.data_ptr()), mode,
                                                  flags, None, C.c_void_p(out.data_ptr()), None, C.c_void_p(ptr), size, None)
    assert lib.frw_groth16_verify_wire_dev(*args(ws.data_ptr(), ws.numel(), mode=2)) == -1
    assert lib.frw_groth16_verify_wire_dev(*args(ws.data_ptr(), ver.wire_workspace_bytes(1, 0, compressed) - 16)) == -1
    assert lib.frw_groth16_verify_wire_dev(*args(ws.data_ptr() + 8, ws.numel() - 8)) == -1
    assert lib.frw_groth16_verify_wire_dev(*args(ws.data_ptr(), ws.numel(), flags=2)) == -1
    assert ver.wire_workspace_bytes(count, 0, compressed) > 0 and lib.frw_groth16_verify_wire_workspace_bytes(ver._h, count, 0, 2) == 0
    torch.cuda.synchronize()
    ver.close()


def test_a_workspace_of_exactly_the_reported_size(oracle):
    """frw_groth16_verify_wire_workspace_bytes is all a call touches: an accepted proof and bytes the decoder refuses in a workspace of
    exactly two proofs' size, bytes of 0xA5 behind it -- accepted and -1, the bytes untouched; one byte short of one proof's is refused."""
    import torch
    import falcon_r1cs_amd as frw
    n = 1025
    k = key(oracle, n)
    inst, limbs = _accepted_and_refused(k, n, 37)
    wire, _ = frw.proofs_to_wire(limbs, True)
    name, bad = next(iter(malformed_cases(True, bytes(wire[0])).items()))
    wire[1] = np.frombuffer(bad, dtype=np.uint8)
    assert frw.proofs_from_wire(wire, True)[1].tolist() == [0, -1], name
    ver = frw.Groth16Verifier(k.limbs(), device=0)
    dev = torch.device("cuda:0")
    d_inst, d_wire = _dev(inst), torch.from_numpy(wire).to(dev)
    buf, ws = T.guarded_workspace(ver.wire_workspace_bytes(2), dev)
    assert ver.verify_wire_dev(d_inst, d_wire, True, workspace=ws).cpu().tolist() == [1, -1]
    assert T.guard_intact(buf)
    with pytest.raises(frw.FrwError) as ei:
        ver.verify_wire_dev(d_inst[:1], d_wire[:1], True, workspace=buf[:ver.wire_workspace_bytes(1) - 1])
    assert ei.value.code == -1
    torch.cuda.synchronize()
    ver.close()


def test_verification_from_wire_bytes_in_a_captured_graph(oracle):
    import torch
    import falcon_r1cs_amd as frw
    n = 1025
    k = key(oracle, n)
    rng = random.Random(29)
    rs = np.random.default_rng(29)
    insts, proofs = [], []
    for b in range(64):
        small = rs.integers(0, 1 << 14, n); small[0] = 1
        p = k.proof(k.dot(small, {}), rng)
        if b % 9 == 4:
            small[7] ^= 1                                                     # a proof of another statement
        insts.append(encode(small, {}, True)); proofs.append(proof_limbs(p))
    want = [0 if b % 9 == 4 else 1 for b in range(64)]
    wire, st = frw.proofs_to_wire(np.stack(proofs))
    assert not st.any()
    wire[20, 47] |= 0xC0                                                      # both flags on A: undecodable
    want[20] = -1
    ver = frw.Groth16Verifier(k.limbs(), device=0)
    dev = torch.device("cuda:0")
    d_inst, d_wire = _dev(np.stack(insts)), torch.from_numpy(wire).to(dev)
    side = torch.cuda.Stream()
    ws = torch.empty(ver.wire_workspace_bytes(64), dtype=torch.uint8, device=dev)
    with torch.cuda.stream(side):
        got = ver.verify_wire_dev(d_inst, d_wire, stream=side.cuda_stream, workspace=ws)
    side.synchronize()
    assert got.cpu().tolist() == want
    torch.cuda.synchronize()
    out = torch.empty(64, dtype=torch.int32, device=dev)
    lib = frw.load_library()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s = torch.cuda.current_stream().cuda_stream
        rc = lib.frw_groth16_verify_wire_dev(ver._h, 64, C.c_void_p(d_inst.data_ptr()), frw.ENC_MONTGOMERY, C.c_void_p(d_wire.data_ptr()), 0, 0,
                                             None, C.c_void_p(out.data_ptr()), None, C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(s))
    assert rc == 0
    out.fill_(7)
    g.replay()
    torch.cuda.synchronize()
    assert out.cpu().tolist() == want
    ver.close()


@pytest.mark.parametrize("logn", [9, 10])
def test_falcon_proofs_through_the_wire_end_to_end(engine, logn):
    import falcon_r1cs_amd as frw
    inst, proofs, vk = _falcon(engine, logn)
    wire, st = frw.proofs_to_wire_dev(proofs)
    assert tuple(wire.shape) == (3, 192) and st.cpu().tolist() == [0, 0, 0]
    ver = frw.Groth16Verifier.from_wire(frw.vk_to_wire(vk), device=0)
    assert ver.verify_wire_dev(inst, wire).cpu().tolist() == [1, 1, 1]
    assert ver.verify_wire_dev(inst, wire, batched=True).cpu().tolist() == [1, 1, 1]
    assert ver.verify_wire_dev(inst[[1, 2, 0]].contiguous(), wire).cpu().tolist() == [0, 0, 0]
    back, st = frw.proofs_from_wire_dev(wire)
    assert st.cpu().tolist() == [0, 0, 0] and bool((back == proofs).all())
    host = frw.Groth16Verifier.from_wire(frw.vk_to_wire(vk, compressed=False), compressed=False)
    assert host.verify(inst.cpu().numpy().view(np.uint64), frw.proofs_from_wire(wire.cpu().numpy())[0]).tolist() == [1, 1, 1]
    host.close()
    ver.close()


@pytest.mark.parametrize("compressed", [True, False])
def test_a_large_key_from_wire_bytes(oracle, compressed):
    import falcon_r1cs_amd as frw
    n = 32769
    k = key(oracle, n)
    rng = random.Random(n)
    rs = np.random.default_rng(n)
    inst, proofs = _batch(k, n, 4, rng, rs, distinct=3)
    other = encode([1], {}, True)[0]
    inst[3, n - 3] = other if not np.array_equal(inst[3, n - 3], other) else encode([2], {}, True)[0]      # the fourth: another statement
    data = frw.vk_to_wire(k.limbs(), compressed)
    assert len(data) == (344 + 48 * n if compressed else 680 + 96 * n)
    ref = frw.Groth16Verifier(k.limbs(), device=0)
    ver = frw.Groth16Verifier.from_wire(data, device=0, compressed=compressed)
    assert ver.num_instance == n
    want = ref.verify_full_dev(_dev(inst), _dev(proofs)).cpu().tolist()
    assert want[:3] == [1, 1, 1] and want[3] == 0
    assert ver.verify_full_dev(_dev(inst), _dev(proofs)).cpu().tolist() == want
    wire, _ = frw.proofs_to_wire(proofs, compressed)
    import torch
    assert ver.verify_wire_dev(_dev(inst), torch.from_numpy(wire).to("cuda:0"), compressed).cpu().tolist() == want
    ref.close()
    ver.close()
    # one undecodable row (x = 1 has no y; uncompressed: off the curve), deep in gamma_abc_g1
    head, g1n = (344, 48) if compressed else (680, 96)
    at = head + g1n * (n - 7)
    row = W._fq(1) if compressed else W._fq(1) + W._fq(1)
    with pytest.raises(frw.FrwError) as ei:
        frw.Groth16Verifier.from_wire(data[:at] + row + data[at + g1n:], device=0, compressed=compressed)
    assert ei.value.code == -1
    # a row that decodes but lies outside the subgroup is the loader's to refuse
    from test_gpu_verify_dev import _stray
    with pytest.raises(frw.FrwError) as ei:
        frw.Groth16Verifier.from_wire(data[:at] + W.g1_encode(_stray(rng), compressed) + data[at + g1n:], device=0, compressed=compressed)
    assert ei.value.code == -1
