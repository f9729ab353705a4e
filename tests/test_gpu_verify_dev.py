"""Groth16 verification with prepare_inputs on the device (falcon-r1cs_amd/csrc/frw_verify_dev.hip): the key's gamma_abc_g1 points
checked on the device, gamma_abc_g1[0] + sum x_i gamma_abc_g1[i] summed there, the rest on host threads.  Checked against the oracle's
fixed-base multiples and bucket sums (oracle/bls12_381.c) and against the host verifier (frw_groth16_verify), verdict for verdict.
Statements are made "in the exponent" as in test_pairing_host.py: gamma_abc_g1[i] = g_i G1, so the prepared point of x is
(sum x_i g_i mod r) G1, and a proof is A = a G1, B = b G2 and C solved for -- no proving key of the aggregate's size is needed."""
import ctypes as C
import random

import numpy as np
import pytest

import frw_testlib as T
from oracle import bls12_381 as E

pytestmark = pytest.mark.gpu

R, Q = E.R, E.Q
RM = (1 << 256) % R                                  # ark-ff's Montgomery form: x -> x 2^256 mod r
BIG = 1571841                                        # the 1,024-statement aggregate's instance count (513 x 1024 + 511 x 2048 + 1)
H1 = 3 * 11 ** 2 * 10177 ** 2 * 859267 ** 2 * 52437899 ** 2      # the cofactor of G1 in E(Fq)
H1_PRIMES = (3, 11, 10177, 859267, 52437899)
_MONT14 = None


def _mont14():
    global _MONT14
    if _MONT14 is None:
        _MONT14 = T.ints_to_limbs([v * RM % R for v in range(1 << 14)])
    return _MONT14


class Key:
    """gamma_abc_g1[i] = g_i G1 (g_i < 2^254; one of them 0: the point at infinity), and the four fixed points."""

    def __init__(self, oracle, n, seed, infinity_at=None):
        rs = np.random.default_rng(seed)
        self.n = n
        self.g = rs.integers(0, 1 << 63, size=(n, 4), dtype=np.int64).view(np.uint64).copy()
        self.g[:, 3] &= np.uint64((1 << 62) - 1)
        if infinity_at is not None:
            self.g[infinity_at] = 0
        self.g16 = self.g.view(np.uint16).reshape(n, 16).astype(np.int64)
        self.gamma_abc = oracle.g1_fixed_base(self.g, threads=16)
        if infinity_at is not None:
            assert not self.gamma_abc[infinity_at].any()
        rng = random.Random(seed)
        self.alpha, self.beta, self.gamma, self.delta = (rng.randrange(1, R) for _ in range(4))
        self.oracle = oracle
        self.fixed = np.concatenate([np.array(E.to_limbs(E.mul(E.G1, self.alpha)), dtype=np.uint64),
                                     np.array(E.g2_to_limbs(E.g2_mul(E.G2, self.beta)), dtype=np.uint64),
                                     np.array(E.g2_to_limbs(E.g2_mul(E.G2, self.gamma)), dtype=np.uint64),
                                     np.array(E.g2_to_limbs(E.g2_mul(E.G2, self.delta)), dtype=np.uint64)])

    def g_int(self, i):
        return int.from_bytes(self.g[i].tobytes(), "little")

    def limbs(self, gamma_abc=None):
        return np.concatenate([self.fixed, (self.gamma_abc if gamma_abc is None else gamma_abc).reshape(-1)])

    def dot(self, small, extra):
        """sum x_i g_i mod r for x = small (ints < 2^14) with x_i replaced by extra[i]: 16-bit pieces of g, exact in int64"""
        small = np.asarray(small, dtype=np.int64).copy()
        for i in extra:
            small[i] = 0
        parts = (small[:, None] * self.g16).sum(axis=0)
        s = sum(int(p) << (16 * j) for j, p in enumerate(parts))
        s += sum(v * self.g_int(i) for i, v in extra.items())
        return s % R

    def point(self, s):
        return self.oracle.g1_fixed_base(T.ints_to_limbs([s]), threads=1)[0]

    def proof(self, acc, rng):
        a, b = rng.randrange(1, R), rng.randrange(1, R)
        c = (a * b - self.alpha * self.beta - self.gamma * acc) * pow(self.delta, -1, R) % R
        return (E.mul(E.G1, a), E.g2_mul(E.G2, b), E.mul(E.G1, c))


def encode(small, extra, montgomery):
    """an instance vector: small values (< 2^14) with full-width ones at the indices of `extra`, uint64[n, 4]"""
    small = np.asarray(small, dtype=np.int64)
    if montgomery:
        out = _mont14()[small].copy()
    else:
        out = np.zeros((small.size, 4), dtype=np.uint64)
        out[:, 0] = small.astype(np.uint64)
    for i, v in extra.items():
        out[i] = T.ints_to_limbs([v * RM % R if montgomery else v])[0]
    return out


def proof_limbs(p):
    return np.array(E.to_limbs(p[0]) + E.g2_to_limbs(p[1]) + E.to_limbs(p[2]), dtype=np.uint64)


def vectors(n, rs):
    """(small, extra) instance vectors of the kinds a verifier meets, the constant one first"""
    out = []
    def one_first(v):
        v = np.asarray(v, dtype=np.int64)
        v[0] = 1
        return v
    out.append((one_first(rs.integers(0, 1 << 14, n)), {}))                 # Falcon-like 14-bit values
    out.append((one_first(np.full(n, 12288)), {}))                          # all q - 1
    out.append((one_first(np.zeros(n)), {}))                                # nothing but the constant
    runs = (np.arange(n) // 97) % 2                                         # long runs of ones
    out.append((one_first(runs), {}))
    out.append((one_first(rs.integers(0, 1 << 14, n)), {int(rs.integers(1, n)): R - 1}))    # one full-width value
    out.append((one_first(rs.integers(0, 2, n)), {}))                       # booleans
    return out


_KEYS = {}


def key(oracle, n):
    if n not in _KEYS:
        _KEYS[n] = Key(oracle, n, seed=n, infinity_at=n // 2)
    return _KEYS[n]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(torch.device("cuda:0"))


@pytest.mark.parametrize("n", [1025, 2049, 32769, BIG])
def test_prepare_inputs_equals_the_oracle(oracle, n):
    import falcon_r1cs_amd as frw
    k = key(oracle, n)
    ver = frw.Groth16Verifier(k.limbs(), device=0)
    rs = np.random.default_rng(7 + n)
    vecs = vectors(n, rs)
    want = [k.point(k.dot(s, e)) for s, e in vecs]
    for montgomery in (True, False):
        inst = np.stack([encode(s, e, montgomery) for s, e in vecs])
        prepared, status = ver.prepare_inputs_dev(_dev(inst), frw.ENC_MONTGOMERY if montgomery else frw.ENC_CANONICAL)
        got = prepared.cpu().numpy().view(np.uint64)
        assert status.cpu().tolist() == [0] * len(vecs)
        for b in range(len(vecs)):
            assert got[b].tolist() == want[b].tolist(), (montgomery, b)
        if n <= 2049:
            for b, (s, e) in enumerate(vecs):
                canon = encode(s, e, False)
                assert got[b].tolist() == oracle.g1_msm(k.gamma_abc, canon, threads=16).tolist(), b
    ver.close()


@pytest.mark.parametrize("montgomery", [True, False])
def test_malformed_instance_vectors_are_flagged_before_the_sum(oracle, montgomery):
    import falcon_r1cs_amd as frw
    n = 1025
    k = key(oracle, n)
    enc = frw.ENC_MONTGOMERY if montgomery else frw.ENC_CANONICAL
    ver = frw.Groth16Verifier(k.limbs(), device=0)
    rs = np.random.default_rng(3)
    good = [encode(s, e, montgomery) for s, e in vectors(n, rs)[:2]]
    bad = []
    v = good[0].copy(); v[5] = T.ints_to_limbs([R])[0]; bad.append(v)                     # a canonical value equal to r
    v = good[0].copy()
    i = next(i for i in range(1, n) if int.from_bytes(v[i].tobytes(), "little") + R < 1 << 256)
    v[i] = T.ints_to_limbs([int.from_bytes(v[i].tobytes(), "little") + R])[0]; bad.append(v)   # the limbs x + r
    v = good[1].copy(); v[0] = encode([2], {}, montgomery)[0]; bad.append(v)             # instance[0] = 2
    v = good[1].copy(); v[0] = 0; bad.append(v)                                          # instance[0] = 0
    inst = np.stack([good[0], bad[0], bad[1], good[1], bad[2], bad[3]])
    prepared, status = ver.prepare_inputs_dev(_dev(inst), enc)
    assert status.cpu().tolist() == [0, -1, -1, 0, -1, -1]
    p_good, s_good = ver.prepare_inputs_dev(_dev(np.stack(good)), enc)
    assert s_good.cpu().tolist() == [0, 0]
    got = prepared.cpu().numpy()
    assert np.array_equal(got[[0, 3]], p_good.cpu().numpy())
    assert not got[[1, 2, 4, 5]].any()
    # and the host says -1 for exactly these
    host = frw.Groth16Verifier(k.limbs())
    pf = np.zeros((6, 48), dtype=np.uint64)
    assert host.verify(inst[[1, 2, 4, 5]], pf[:4], enc).tolist() == [-1] * 4
    host.close()
    ver.close()


def _stray(rng):
    """a point of E(Fq) outside G1"""
    while True:
        x = rng.randrange(Q)
        y2 = (x ** 3 + 4) % Q
        y = pow(y2, (Q + 1) // 4, Q)
        if y * y % Q == y2 and E.add(E.mul((x, y), R - 1), (x, y)) is not None:
            return (x, y)


def _torsion(rng, ell):
    """a point of order ell (a prime dividing the cofactor): r Q for a random curve point Q lies in E[h1]; (h1 / ell^e) (r Q) in its
    ell-part (which need not be cyclic: ell^e is the whole power of ell in h1), multiplied by ell while that leaves a point"""
    e = 1
    while H1 % ell ** (e + 1) == 0:
        e += 1
    while True:
        q = _stray(rng)
        rq = E.add(E.mul(q, R - 1), q)                               # (E.mul reduces its scalar mod r)
        p = E.mul(rq, H1 // ell ** e)
        if p is None:
            continue
        while E.mul(p, ell) is not None:
            p = E.mul(p, ell)
        return p


def _plus_q(limbs6):
    v = int.from_bytes(np.asarray(limbs6, dtype=np.uint64).tobytes(), "little") + Q
    return np.frombuffer(v.to_bytes(48, "little"), dtype=np.uint64)


@pytest.mark.parametrize("montgomery", [True, False])
def test_verdicts_equal_the_host_verifiers_in_one_mixed_batch(oracle, montgomery):
    import falcon_r1cs_amd as frw
    n = 1025
    k = key(oracle, n)
    enc = frw.ENC_MONTGOMERY if montgomery else frw.ENC_CANONICAL
    rng = random.Random(11)
    rs = np.random.default_rng(11)
    small = rs.integers(0, 1 << 14, n); small[0] = 1
    proof = k.proof(k.dot(small, {}), rng)
    x = encode(small, {}, montgomery)
    good = proof_limbs(proof)
    cases = [(x, good)]                                                       # accepted
    x2 = small.copy(); x2[3] = (x2[3] + 1) % (1 << 14)
    cases.append((encode(x2, {}, montgomery), good))                           # another statement
    cases.append((x, proof_limbs((E.mul(proof[0], 2), proof[1], proof[2]))))   # A, B, C tampered with
    cases.append((x, proof_limbs((proof[0], E.g2_mul(proof[1], 3), proof[2]))))
    cases.append((x, proof_limbs((proof[0], proof[1], E.add(proof[2], E.G1)))))
    cases.append((x, proof_limbs((None, proof[1], proof[2]))))                 # A = O
    v = x.copy(); v[0] = encode([2], {}, montgomery)[0]; cases.append((v, good))   # the constant is not one
    v = x.copy(); v[3] = T.ints_to_limbs([R])[0]; cases.append((v, good))     # a value >= r
    off = good.copy(); off[12] ^= np.uint64(1); cases.append((x, off))        # a coordinate off its curve
    for first in (0, 12, 42):                                                 # x + q aliases (A.x, B.x.c0, C.y)
        alias = good.copy(); alias[first:first + 6] = _plus_q(good[first:first + 6]); cases.append((x, alias))
    cases.append((x, proof_limbs((_stray(rng), proof[1], proof[2]))))          # A outside G1
    inst = np.stack([c[0] for c in cases])
    proofs = np.stack([c[1] for c in cases])
    host = frw.Groth16Verifier(k.limbs())
    ver = frw.Groth16Verifier(k.limbs(), device=0)
    d_inst, d_proofs = _dev(inst), _dev(proofs)
    for flags in (0, frw.VERIFY_POINTS_ARE_CHECKED):
        want = host.verify(inst, proofs, enc, flags).tolist()
        assert ver.verify_dev(d_inst, d_proofs, enc, flags).tolist() == want, flags
        assert ver.verify(inst, proofs, enc, flags).tolist() == want          # the device key serves the host path unchanged
    assert host.verify(inst, proofs, enc).tolist() == [1, 0, 0, 0, 0, 0, -1, -1, -1, -1, -1, -1, -1]
    assert host.verify(inst, proofs, enc, frw.VERIFY_POINTS_ARE_CHECKED).tolist()[-1] == 0
    host.close()
    ver.close()


@pytest.mark.parametrize("logn", [9, 10])
def test_falcon_proofs_end_to_end_from_device_buffers(engine, logn):
    import torch
    import falcon_r1cs_amd as frw
    dev = torch.device("cuda:0")
    batch = 3
    L = frw.layout(logn)
    rng = random.Random(900 + logn)
    pk, vk = engine.groth16_setup(0, logn, *(rng.randrange(2, R) for _ in range(5)))
    r1cs = engine.r1cs_load(0, logn)
    try:
        sig, pk_, hm = frw.synth_triples(logn, batch, seed=31 + logn)
        dd = [torch.from_numpy(a.view(np.int16)).to(dev) for a in (sig, pk_, hm)]
        wit = torch.empty((batch, L.num_witness, 4), dtype=torch.int64, device=dev)
        inst = torch.empty((batch, L.num_instance, 4), dtype=torch.int64, device=dev)
        st = torch.empty(batch, dtype=torch.int32, device=dev)
        s0 = torch.cuda.current_stream().cuda_stream
        engine.witness_ntt_verify_dev(logn, batch, dd[0], dd[1], dd[2], wit, inst, st, frw.ENC_MONTGOMERY, s0)
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0
        # proof 2 from a witness that violates the system (one boolean flipped after the witness kernel ran)
        w2 = wit[2, L.seg_off[2]].clone()
        one = torch.from_numpy(np.frombuffer(RM.to_bytes(32, "little"), dtype=np.int64).copy()).to(dev)
        wit[2, L.seg_off[2]] = torch.where(w2.abs().sum() == 0, one, torch.zeros_like(one))
        rs = np.array([T.ints_to_limbs([rng.randrange(R), rng.randrange(R)]) for _ in range(batch)])
        ws_bytes = engine.groth16_workspace_bytes(pk, r1cs, batch)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        proofs = torch.empty((batch, 48), dtype=torch.int64, device=dev)
        engine.groth16_prove_dev(pk, r1cs, batch, wit, inst, rs, proofs, ws, ws_bytes, None, s0)
        torch.cuda.synchronize()
        ver = frw.Groth16Verifier(vk, device=0)
        host = frw.Groth16Verifier(vk)
        inst_h, proofs_h = inst.cpu().numpy().view(np.uint64), proofs.cpu().numpy().view(np.uint64)
        got = ver.verify_dev(inst, proofs, frw.ENC_MONTGOMERY, stream=s0)
        assert got.tolist() == [1, 1, 0]
        assert got.tolist() == host.verify(inst_h, proofs_h).tolist()
        perm = inst[[1, 0, 2]].contiguous()
        got = ver.verify_dev(perm, proofs, frw.ENC_MONTGOMERY, stream=s0)
        assert got.tolist() == [0, 0, 0]
        assert got.tolist() == host.verify(inst_h[[1, 0, 2]], proofs_h).tolist()
        ver.close()
        host.close()
    finally:
        engine.r1cs_free(r1cs)
        engine.groth16_pk_free(pk)


def test_aggregate_size_statement_is_accepted_and_its_last_input_counts(oracle):
    import falcon_r1cs_amd as frw
    k = key(oracle, BIG)
    rng = random.Random(44)
    rs = np.random.default_rng(44)
    small = rs.integers(0, 1 << 14, BIG); small[0] = 1
    proof = proof_limbs(k.proof(k.dot(small, {}), rng))
    changed = small.copy(); changed[BIG - 3] = (changed[BIG - 3] + 1) % (1 << 14)
    ver = frw.Groth16Verifier(k.limbs(), device=0)
    inst = np.stack([encode(small, {}, True), encode(changed, {}, True)])
    got = ver.verify_dev(_dev(inst), _dev(np.stack([proof, proof])), frw.ENC_MONTGOMERY)
    assert got.tolist() == [1, 0]
    ver.close()


def _bad_points(rng, base_point):
    """(name, 12 limbs) of rows a key must not hold; base_point: a G1 point to add a torsion point to"""
    out = []
    good = np.array(E.to_limbs(base_point), dtype=np.uint64)
    alias = good.copy(); alias[:6] = _plus_q(good[:6]); out.append(("x + q", alias))
    off = good.copy(); off[6] ^= np.uint64(1); out.append(("off the curve", off))
    for ell in H1_PRIMES:
        t = _torsion(rng, ell)
        out.append(("order %d" % ell, np.array(E.to_limbs(t), dtype=np.uint64)))
        out.append(("G1 + order %d" % ell, np.array(E.to_limbs(E.add(base_point, t)), dtype=np.uint64)))
    return out


def test_key_points_are_checked_on_the_device(oracle):
    import falcon_r1cs_amd as frw
    n = 1025
    k = key(oracle, n)
    rng = random.Random(17)
    base = E.mul(E.G1, 12345)
    bad = _bad_points(rng, base)
    ver = frw.Groth16Verifier(k.limbs(), device=0)                             # the valid key loads
    ver.close()
    with pytest.raises(frw.FrwError) as ei:
        frw.Groth16Verifier(k.limbs(), points_are_checked=True, device=0)      # vouching is refused
    assert ei.value.code == -1
    for pos in (1, n // 2 + 1, n - 1):
        for name, row in bad:
            g = k.gamma_abc.copy()
            g[pos] = row
            with pytest.raises(frw.FrwError) as ei:
                frw.Groth16Verifier(k.limbs(g), device=0)
            assert ei.value.code == -1, (pos, name)
            with pytest.raises(frw.FrwError):
                frw.Groth16Verifier(k.limbs(g))                                 # the host load refuses the same keys
    # the aggregate-size key: one bad point at its last index
    kb = key(oracle, BIG)
    g = kb.gamma_abc.copy()
    g[BIG - 1] = bad[2][1]
    with pytest.raises(frw.FrwError):
        frw.Groth16Verifier(kb.limbs(g), device=0)


def test_workspace_chunks_and_refusals(oracle):
    import torch
    import falcon_r1cs_amd as frw
    n = 1025
    k = key(oracle, n)
    rng = random.Random(23)
    rs = np.random.default_rng(23)
    insts, proofs = [], []
    for b in range(5):
        small = rs.integers(0, 1 << 14, n); small[0] = 1
        p = k.proof(k.dot(small, {}), rng)
        if b == 3:
            small[7] ^= 1                                                     # a proof of another statement
        insts.append(encode(small, {}, True)); proofs.append(proof_limbs(p))
    ver = frw.Groth16Verifier(k.limbs(), device=0)
    d_inst, d_proofs = _dev(np.stack(insts)), _dev(np.stack(proofs))
    dev = torch.device("cuda:0")
    ws5 = torch.empty(ver.workspace_bytes(5), dtype=torch.uint8, device=dev)
    ws2 = torch.empty(ver.workspace_bytes(2), dtype=torch.uint8, device=dev)
    assert ver.workspace_bytes(2) < ver.workspace_bytes(5)
    full = ver.verify_dev(d_inst, d_proofs, workspace=ws5)
    assert full.tolist() == [1, 1, 1, 0, 1]
    assert ver.verify_dev(d_inst, d_proofs, workspace=ws2).tolist() == full.tolist()
    p5, s5 = ver.prepare_inputs_dev(d_inst, workspace=ws5)
    p2, s2 = ver.prepare_inputs_dev(d_inst, workspace=ws2)
    assert torch.equal(p5, p2) and torch.equal(s5, s2)
    lib = frw.load_library()
    acc = np.zeros(5, dtype=np.int32)
    one = ver.workspace_bytes(1)
    args = lambda ptr, size: (ver._h, 5, C.c_void_p(d_inst.data_ptr()), frw.ENC_MONTGOMERY, C.c_void_p(d_proofs.data_ptr()), 0,
                              acc.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), size, None)
    assert lib.frw_groth16_verify_dev(*args(ws5.data_ptr(), one - 16)) == -1                 # too small for one proof
    assert lib.frw_groth16_verify_dev(*args(ws5.data_ptr() + 8, ws5.numel() - 8)) == -1     # misaligned
    out_p = torch.empty((5, 12), dtype=torch.int64, device=dev)
    out_s = torch.empty(5, dtype=torch.int32, device=dev)
    pargs = lambda ptr, size: (ver._h, 5, C.c_void_p(d_inst.data_ptr()), frw.ENC_MONTGOMERY, C.c_void_p(out_p.data_ptr()),
                               C.c_void_p(out_s.data_ptr()), C.c_void_p(ptr), size, None)
    assert lib.frw_groth16_prepare_inputs_dev(*pargs(ws5.data_ptr(), one - 16)) == -1
    assert lib.frw_groth16_prepare_inputs_dev(*pargs(ws5.data_ptr() + 8, ws5.numel() - 8)) == -1
    assert lib.frw_groth16_verify_dev(*args(ws5.data_ptr(), ws5.numel())) == 0
    assert acc.tolist() == full.tolist()
    ver.close()
