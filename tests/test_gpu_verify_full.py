"""Groth16 verification entirely on the device (frw_groth16_verify_full_dev, frw_pairing_dev.hip): the pairing against the host's
frw_diag_pairing value for value, and the verdicts against frw_groth16_verify entry for entry.  Statements are made "in the exponent"
as in test_gpu_verify_dev.py, whose key and proof helpers are used here."""
import ctypes as C
import random

import numpy as np
import pytest

import frw_testlib as T
from oracle import bls12_381 as E
from test_gpu_verify_dev import BIG, R, _dev, _plus_q, _stray, encode, key, proof_limbs

pytestmark = pytest.mark.gpu


def _g1(p):
    return np.array(E.to_limbs(p), dtype=np.uint64)


def _g2(p):
    return np.array(E.g2_to_limbs(p), dtype=np.uint64)


H2 = 0x5d543a95414e7f1091d50792876a202cd91de4547085abaa68a205b2e5a7ddfa628f1cb4d9e82ef21537e293a6691ae1616ec6e786f0c70cf1c38e31c7238e5
Q = E.Q                                              # (H2: the cofactor of G2 in E'(Fq2), #E' = H2 r)


def _fsqrt(a):
    r = pow(a, (Q + 1) // 4, Q)
    return r if r * r % Q == a % Q else None


def _f2_sqrt(a):
    """a square root in Fq2 (q = 3 mod 4), or None"""
    a0, a1 = a[0] % Q, a[1] % Q
    n = _fsqrt((a0 * a0 + a1 * a1) % Q)
    if n is None:
        return None
    half = pow(2, -1, Q)
    for t in ((a0 + n) * half % Q, (a0 - n) * half % Q):
        c0 = _fsqrt(t)
        if c0:
            c = (c0, a1 * pow(2 * c0, -1, Q) % Q)
            if E.f2_mul(c, c) == (a0, a1):
                return c
    return None


def _g2_mul_full(p, k):
    """k P on the twist without reducing k mod r (E.g2_mul does)"""
    acc = None
    while k:
        if k & 1:
            acc = E.g2_add(acc, p)
        p = E.g2_add(p, p)
        k >>= 1
    return acc


def _twist_point(rng):
    """a point of E'(Fq2): y^2 = x^3 + 4 (1 + u), almost surely outside G2"""
    while True:
        x = (rng.randrange(Q), rng.randrange(Q))
        y = _f2_sqrt(E.f2_add(E.f2_mul(E.f2_mul(x, x), x), (4, 4)))
        if y:
            assert _g2_mul_full((x, y), E.R) is not None and _g2_mul_full((x, y), H2 * E.R) is None
            return (x, y)


def _twist_order_13(rng):
    """a point of order 13 on the twist: in the Miller loop over |z| it meets T = -Q (2 T = -Q before an addition), a vertical line"""
    while True:
        p = _g2_mul_full(_twist_point(rng), H2 * E.R // 13 ** 2)
        if p is not None and _g2_mul_full(p, 13) is not None:
            p = _g2_mul_full(p, 13)
        if p is not None:
            assert _g2_mul_full(p, 13) is None
            return p


def test_device_pairing_equals_the_hosts():
    import falcon_r1cs_amd as frw
    rng = random.Random(5)
    g1s = [E.G1, E.mul(E.G1, R - 1), None, E.G1]
    g2s = [E.G2, E.G2, E.G2, None]
    for _ in range(64):
        s = rng.randrange(1, R)
        p = E.mul(E.G1, rng.randrange(1, R))
        g1s += [p]
        g2s += [E.g2_mul(E.G2, s)]
    g1s += [E.mul(g1s[-1], R - 1)]                                           # -P against the same Q
    g2s += [g2s[-2]]
    a = np.stack([_g1(p) for p in g1s])
    b = np.stack([_g2(q) for q in g2s])
    got = frw.diag_pairing_dev(a, b)
    for i in range(len(g1s)):
        assert np.array_equal(got[i], frw.diag_pairing(a[i], b[i])), i
    # bilinearity: e(x P, y Q) = e(x y P, Q)
    x, y = rng.randrange(1, R), rng.randrange(1, R)
    lhs = frw.diag_pairing_dev(np.stack([_g1(E.mul(E.G1, x)), _g1(E.mul(E.G1, x * y % R))]),
                               np.stack([_g2(E.g2_mul(E.G2, y)), _g2(E.G2)]))
    assert np.array_equal(lhs[0], lhs[1])
    # a point off its curve is refused, as by the host
    off = _g1(E.G1).copy()
    off[6] ^= np.uint64(1)
    with pytest.raises(frw.FrwError) as ei:
        frw.diag_pairing_dev(off[None], _g2(E.G2)[None])
    assert ei.value.code == -1


def _mixed_cases(k, n, montgomery, rng, rs):
    small = rs.integers(0, 1 << 14, n); small[0] = 1
    proof = k.proof(k.dot(small, {}), rng)
    x = encode(small, {}, montgomery)
    good = proof_limbs(proof)
    cases = [(x, good)]                                                       # accepted
    small2 = rs.integers(0, 1 << 14, n); small2[0] = 1
    cases.append((encode(small2, {}, montgomery), proof_limbs(k.proof(k.dot(small2, {}), rng))))   # another accepted one
    x2 = small.copy(); x2[3] = (x2[3] + 1) % (1 << 14)
    cases.append((encode(x2, {}, montgomery), good))                           # a wrong statement
    cases.append((x, proof_limbs((E.mul(proof[0], 2), proof[1], proof[2]))))   # A, B, C altered
    cases.append((x, proof_limbs((proof[0], E.g2_mul(proof[1], 3), proof[2]))))
    cases.append((x, proof_limbs((proof[0], proof[1], E.add(proof[2], E.G1)))))
    cases.append((x, proof_limbs((None, proof[1], proof[2]))))                 # points at infinity
    cases.append((x, proof_limbs((proof[0], None, proof[2]))))
    cases.append((x, proof_limbs((proof[0], proof[1], None))))
    v = x.copy(); v[0] = encode([2], {}, montgomery)[0]; cases.append((v, good))   # instance[0] != 1
    v = x.copy(); v[3] = T.ints_to_limbs([R])[0]; cases.append((v, good))     # an instance value >= r
    off = good.copy(); off[12] ^= np.uint64(1); cases.append((x, off))        # B off its curve
    off = good.copy(); off[6] ^= np.uint64(1); cases.append((x, off))         # A off its curve
    off = good.copy(); off[42] ^= np.uint64(1); cases.append((x, off))        # C off its curve
    for first in (0, 12, 42):                                                 # a coordinate >= q (x + q)
        alias = good.copy(); alias[first:first + 6] = _plus_q(good[first:first + 6]); cases.append((x, alias))
    cases.append((x, proof_limbs((_stray(rng), proof[1], proof[2]))))          # A, C outside G1
    cases.append((x, proof_limbs((proof[0], proof[1], _stray(rng)))))
    cases.append((x, proof_limbs((proof[0], _twist_point(rng), proof[2]))))    # B outside G2
    cases.append((x, proof_limbs((proof[0], _twist_order_13(rng), proof[2]))))   # B of order 13: a degenerate loop when vouched for
    cases.append((x, proof_limbs((None, _twist_order_13(rng), proof[2]))))     # ... whose pair drops out with A = O
    return cases


@pytest.mark.parametrize("montgomery", [True, False])
def test_verdicts_equal_the_host_verifiers_in_one_mixed_batch(oracle, montgomery):
    import falcon_r1cs_amd as frw
    n = 1025
    k = key(oracle, n)
    enc = frw.ENC_MONTGOMERY if montgomery else frw.ENC_CANONICAL
    cases = _mixed_cases(k, n, montgomery, random.Random(11), np.random.default_rng(11))
    inst = np.stack([c[0] for c in cases])
    proofs = np.stack([c[1] for c in cases])
    host = frw.Groth16Verifier(k.limbs())
    ver = frw.Groth16Verifier(k.limbs(), device=0)
    d_inst, d_proofs = _dev(inst), _dev(proofs)
    for flags in (0, frw.VERIFY_POINTS_ARE_CHECKED):
        want = host.verify(inst, proofs, enc, flags).tolist()
        got = ver.verify_full_dev(d_inst, d_proofs, enc, flags)
        assert got.is_cuda and str(got.dtype) == "torch.int32"
        assert got.cpu().tolist() == want, flags
    strict, vouched = host.verify(inst, proofs, enc).tolist(), host.verify(inst, proofs, enc, frw.VERIFY_POINTS_ARE_CHECKED).tolist()
    assert strict[:3] == [1, 1, 0]
    assert strict[-5:] == [-1] * 5                                            # every point outside its subgroup is refused ...
    assert vouched[-5:] == [0, 0, 0, -1, 0]                                   # ... or, vouched for, just fails (the vertical line: -1)
    host.close()
    ver.close()


@pytest.mark.parametrize("logn", [9, 10])
def test_falcon_proofs_end_to_end_from_device_buffers(engine, logn):
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    batch = 3
    L = frw.layout(logn)
    rng = random.Random(700 + logn)
    pk, vk = engine.groth16_setup(0, logn, *(rng.randrange(2, R) for _ in range(5)))
    r1cs = engine.r1cs_load(0, logn)
    try:
        sig, pk_, hm = frw.synth_triples(logn, batch, seed=41 + logn)
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
        ver = frw.Groth16Verifier(vk, device=0)
        got = ver.verify_full_dev(inst, proofs, frw.ENC_MONTGOMERY, stream=s0)
        assert got.cpu().tolist() == [1, 1, 1]
        perm = inst[[1, 2, 0]].contiguous()                                   # the same proofs against other statements
        assert ver.verify_full_dev(perm, proofs, frw.ENC_MONTGOMERY, stream=s0).cpu().tolist() == [0, 0, 0]
        host = frw.Groth16Verifier(vk)
        assert host.verify(perm.cpu().numpy().view(np.uint64), proofs.cpu().numpy().view(np.uint64)).tolist() == [0, 0, 0]
        ver.close()
        host.close()
    finally:
        engine.r1cs_free(r1cs)
        engine.groth16_pk_free(pk)


def test_large_keys(oracle):
    import falcon_r1cs_amd as frw
    for n, count in ((32769, 4), (BIG, 1)):
        k = key(oracle, n)
        rng = random.Random(n)
        rs = np.random.default_rng(n)
        insts, proofs = [], []
        for _ in range(count):
            small = rs.integers(0, 1 << 14, n); small[0] = 1
            insts.append(encode(small, {}, True)); proofs.append(proof_limbs(k.proof(k.dot(small, {}), rng)))
        changed = insts[0].copy(); changed[n - 3] = encode([int(rs.integers(1, 1 << 14))], {}, True)[0]
        if np.array_equal(changed, insts[0]):
            changed[n - 3] = encode([0], {}, True)[0]
        insts.append(changed); proofs.append(proofs[0])
        ver = frw.Groth16Verifier(k.limbs(), device=0)
        got = ver.verify_full_dev(_dev(np.stack(insts)), _dev(np.stack(proofs)), frw.ENC_MONTGOMERY)
        assert got.cpu().tolist() == [1] * count + [0], n
        ver.close()


def test_streams_graph_capture_and_chunks(oracle):
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
    ver = frw.Groth16Verifier(k.limbs(), device=0)
    dev = torch.device("cuda:0")
    d_inst, d_proofs = _dev(np.stack(insts)), _dev(np.stack(proofs))
    assert ver.verify_full_dev(d_inst, d_proofs).cpu().tolist() == want
    # a workspace for 7 proofs: the batch in chunks
    ws7 = torch.empty(ver.full_workspace_bytes(7), dtype=torch.uint8, device=dev)
    assert ver.full_workspace_bytes(7) < ver.full_workspace_bytes(64)
    assert ver.verify_full_dev(d_inst, d_proofs, workspace=ws7).cpu().tolist() == want
    # on a side stream, then captured into a single-stream graph and replayed
    side = torch.cuda.Stream()
    ws = torch.empty(ver.full_workspace_bytes(64), dtype=torch.uint8, device=dev)
    out = torch.empty(64, dtype=torch.int32, device=dev)
    with torch.cuda.stream(side):
        got = ver.verify_full_dev(d_inst, d_proofs, stream=side.cuda_stream, workspace=ws)
    side.synchronize()
    assert got.cpu().tolist() == want
    torch.cuda.synchronize()
    lib = frw.load_library()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s = torch.cuda.current_stream().cuda_stream
        rc = lib.frw_groth16_verify_full_dev(ver._h, 64, C.c_void_p(d_inst.data_ptr()), frw.ENC_MONTGOMERY, C.c_void_p(d_proofs.data_ptr()), 0,
                                             None, C.c_void_p(out.data_ptr()), None, C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(s))
    assert rc == 0
    out.fill_(7)
    g.replay()
    torch.cuda.synchronize()
    assert out.cpu().tolist() == want
    # refusals: too small, misaligned, a batched request without a seed
    args = lambda ptr, size, flags=0: (ver._h, 64, C.c_void_p(d_inst.data_ptr()), frw.ENC_MONTGOMERY, C.c_void_p(d_proofs.data_ptr()), flags,
                                       None, C.c_void_p(out.data_ptr()), None, C.c_void_p(ptr), size, None)
    assert lib.frw_groth16_verify_full_dev(*args(ws.data_ptr(), ver.full_workspace_bytes(1) - 16)) == -1
    assert lib.frw_groth16_verify_full_dev(*args(ws.data_ptr() + 8, ws.numel() - 8)) == -1
    assert lib.frw_groth16_verify_full_dev(*args(ws.data_ptr(), ws.numel(), 2)) == -1
    torch.cuda.synchronize()
    ver.close()


def _accepted_and_refused(k, n, seed):
    """two cases for the key: a proof that verifies, and the same with A off its curve (refused: -1) -- (instances, proofs' limbs)"""
    rng, rs = random.Random(seed), np.random.default_rng(seed)
    small = rs.integers(0, 1 << 14, n); small[0] = 1
    good = proof_limbs(k.proof(k.dot(small, {}), rng))
    off = good.copy(); off[6] ^= np.uint64(1)
    x = encode(small, {}, True)
    return np.stack([x, x]), np.stack([good, off])


def test_a_workspace_of_exactly_the_reported_size(oracle):
    """frw_groth16_verify_full_workspace_bytes is all a call touches: an accepted and a refused proof in a workspace of exactly two proofs'
    size, bytes of 0xA5 behind it -- the host's verdicts, the bytes untouched; one byte short of one proof's is refused (FRW_E_INVALID_ARG)."""
    import torch
    import falcon_r1cs_amd as frw
    n = 1025
    k = key(oracle, n)
    inst, proofs = _accepted_and_refused(k, n, 31)
    host = frw.Groth16Verifier(k.limbs())
    want = host.verify(inst, proofs).tolist()
    host.close()
    assert want == [1, -1]
    ver = frw.Groth16Verifier(k.limbs(), device=0)
    dev = torch.device("cuda:0")
    d_inst, d_proofs = _dev(inst), _dev(proofs)
    buf, ws = T.guarded_workspace(ver.full_workspace_bytes(2), dev)
    assert ver.verify_full_dev(d_inst, d_proofs, workspace=ws).cpu().tolist() == want
    assert T.guard_intact(buf)
    with pytest.raises(frw.FrwError) as ei:
        ver.verify_full_dev(d_inst[:1], d_proofs[:1], workspace=buf[:ver.full_workspace_bytes(1) - 1])
    assert ei.value.code == -1
    torch.cuda.synchronize()
    ver.close()


def test_a_key_with_gamma_at_infinity(oracle):
    """a pair whose fixed G2 point is the point at infinity contributes one, on the host and on the device alike"""
    import falcon_r1cs_amd as frw
    n = 1025
    k = key(oracle, n)
    rng = random.Random(61)
    limbs = k.limbs().copy()
    limbs[36:60] = 0                                                          # gamma_g2 = O
    proofs = []
    for tamper in (0, 1):
        a, b = rng.randrange(1, R), rng.randrange(1, R)
        c = (a * b - k.alpha * k.beta) * pow(k.delta, -1, R) % R              # e(P, -gamma) = 1 whatever the statement
        proofs.append(proof_limbs((E.mul(E.G1, a), E.g2_mul(E.G2, b), E.mul(E.G1, c + tamper))))
    rs = np.random.default_rng(61)
    small = rs.integers(0, 1 << 14, n); small[0] = 1
    inst = np.stack([encode(small, {}, True)] * 2)
    host = frw.Groth16Verifier(limbs)
    ver = frw.Groth16Verifier(limbs, device=0)
    want = host.verify(inst, np.stack(proofs)).tolist()
    assert want == [1, 0]
    assert ver.verify_full_dev(_dev(inst), _dev(np.stack(proofs))).cpu().tolist() == want
    assert ver.verify_full_dev(_dev(inst), _dev(np.stack(proofs)), batched=True).cpu().tolist() == want
    host.close()
    ver.close()


def _batch(k, n, count, rng, rs, distinct=16):
    insts, proofs = [], []
    for _ in range(distinct):
        small = rs.integers(0, 1 << 14, n); small[0] = 1
        insts.append(encode(small, {}, True)); proofs.append(proof_limbs(k.proof(k.dot(small, {}), rng)))
    idx = [i % distinct for i in range(count)]
    return np.stack([insts[i] for i in idx]), np.stack([proofs[i] for i in idx])


def test_batched_check(oracle):
    import torch
    import falcon_r1cs_amd as frw
    n = 1025
    k = key(oracle, n)
    rng = random.Random(71)
    rs = np.random.default_rng(71)
    inst, proofs = _batch(k, n, 256, rng, rs)
    ver = frw.Groth16Verifier(k.limbs(), device=0)
    host = frw.Groth16Verifier(k.limbs())
    dev = torch.device("cuda:0")
    passed = torch.full((1,), 7, dtype=torch.int32, device=dev)
    seeds = [np.array([1, 2, 3, 4], dtype=np.uint64), np.array([2 ** 64 - 1, 5, 0, 9], dtype=np.uint64)]
    # 256 valid proofs
    d_inst, d_proofs = _dev(inst), _dev(proofs)
    for seed in seeds:
        assert ver.verify_full_dev(d_inst, d_proofs, batched=True, seed=seed, batch_passed=passed).cpu().tolist() == [1] * 256
        assert passed.item() == 1
    # one invalid proof at a random position: exactly that entry 0, the batched check failed
    pos = rng.randrange(256)
    bad = proofs.copy()
    bad[pos] = proof_limbs((E.mul(E.G1, 5), E.G2, E.mul(E.G1, 7)))
    want = [0 if i == pos else 1 for i in range(256)]
    for seed in seeds:
        assert ver.verify_full_dev(d_inst, _dev(bad), batched=True, seed=seed, batch_passed=passed).cpu().tolist() == want
        assert passed.item() == 0
    # a malformed proof (A off its curve) and a malformed statement: -1 for them, and the rest pass together
    mal = proofs.copy()
    mal[3, 6] ^= np.uint64(1)
    mal_inst = inst.copy()
    mal_inst[200, 0] = encode([2], {}, True)[0]
    want = host.verify(mal_inst, mal).tolist()
    assert want == [-1 if i in (3, 200) else 1 for i in range(256)]
    for seed in seeds:
        assert ver.verify_full_dev(_dev(mal_inst), _dev(mal), batched=True, seed=seed, batch_passed=passed).cpu().tolist() == want
        assert passed.item() == 1
    # in chunks: a workspace for 7 proofs runs 37 passes, batch_passed is their conjunction; a fresh random seed (None) is drawn
    ws7 = torch.empty(ver.full_workspace_bytes(7, frw.VERIFY_BATCHED), dtype=torch.uint8, device=dev)
    assert ver.full_workspace_bytes(7, frw.VERIFY_BATCHED) > ver.full_workspace_bytes(7)
    assert ver.verify_full_dev(d_inst, d_proofs, batched=True, workspace=ws7, batch_passed=passed).cpu().tolist() == [1] * 256
    assert passed.item() == 1
    want = [0 if i == pos else 1 for i in range(256)]
    assert ver.verify_full_dev(d_inst, _dev(bad), batched=True, workspace=ws7, batch_passed=passed).cpu().tolist() == want
    assert passed.item() == 0
    # the mixed batch of the per-proof test, batched: the same verdicts under both flags
    cases = _mixed_cases(k, n, True, random.Random(11), np.random.default_rng(11))
    mi, mp_ = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    for flags in (0, frw.VERIFY_POINTS_ARE_CHECKED):
        assert ver.verify_full_dev(_dev(mi), _dev(mp_), flags=flags, batched=True).cpu().tolist() == host.verify(mi, mp_, frw.ENC_MONTGOMERY, flags).tolist()
    ver.close()
    host.close()
