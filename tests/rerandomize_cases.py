"""The case list of the re-randomisation tests (frw_groth16_rerandomize and its device forms), shared by tests/test_rerandomize_host.py
and tests/test_gpu_rerandomize.py and built once: a synthetic key (Key of test_gpu_verify_dev.py, three instance values), proofs with
known exponents A = a G1, B = b G2, C = c G1, delta_g2 = d G2, and the expected points from oracle/bls12_381.py's affine arithmetic in
Python integers:
    A' = (1 / r1) A        B' = r1 B + (r1 r2 mod r) delta_g2        C' = C + r2 A
An affine point has one representation, so every comparison is bit for bit."""
import random

import numpy as np

import frw_testlib as T
from oracle import bls12_381 as E
from test_gpu_verify_dev import Key, proof_limbs, _stray, _plus_q
from test_gpu_verify_full import _twist_point

R, Q = E.R, E.Q
LAMBDA = 0xac45a4010001a40200000000ffffffff
EDGES = (1, 2, 3, LAMBDA - 1, LAMBDA, LAMBDA + 1, 2 * LAMBDA, 1 << 127, (1 << 128) - 1, R - 2, R - 1)
ZERO_FACTOR = -2
N_INSTANCE = 3
UNSPECIFIED = "unspecified"           # the output for a point vouched for wrongly: status 0, some point, the same every time


class Case:
    def __init__(self, name, proof, r1, r2, status=0, want=None, status_vouched=None, want_vouched=None):
        self.name, self.proof, self.r1, self.r2 = name, np.asarray(proof, dtype=np.uint64), r1, r2
        self.status, self.want = status, want
        self.status_vouched = status if status_vouched is None else status_vouched
        self.want_vouched = want if want_vouched is None else want_vouched

    @property
    def factors(self):
        return T.ints_to_limbs([self.r1, self.r2])


def expected(points, delta2, r1, r2):
    a, b, c = points
    return proof_limbs((E.mul(a, pow(r1 % R, -1, R)), E.g2_add(E.g2_mul(b, r1), E.g2_mul(delta2, r1 * r2 % R)), E.add(c, E.mul(a, r2))))


class Cases:
    def __init__(self, oracle):
        rng = random.Random(2024)
        self.key = Key(oracle, N_INSTANCE, seed=77)
        k = self.key
        self.delta2 = E.g2_mul(E.G2, k.delta)
        self.statement = [rng.randrange(R) for _ in range(N_INSTANCE - 1)]
        self.acc = (k.g_int(0) + sum(x * k.g_int(i + 1) for i, x in enumerate(self.statement))) % R
        zeros = np.zeros(48, dtype=np.uint64)
        cases = []

        def rand_points():
            return (E.mul(E.G1, rng.randrange(1, R)), E.g2_mul(E.G2, rng.randrange(1, R)), E.mul(E.G1, rng.randrange(1, R)))

        def good(name, pts, r1, r2):
            cases.append(Case(name, proof_limbs(pts), r1, r2, 0, expected(pts, self.delta2, r1, r2)))

        # 1. random factors; the first on a proof that verifies
        self.valid_proof = k.proof(self.acc, rng)
        good("random-valid", self.valid_proof, rng.randrange(1, R), rng.randrange(1, R))
        for i in range(2):
            good("random-%d" % i, rand_points(), rng.randrange(1, R), rng.randrange(1, R))
        # 2. factors >= r
        pts = rand_points()
        good("five", pts, 5, 7)
        good("r-plus-five", pts, R + 5, R + 7)
        good("all-ones", pts, (1 << 256) - 1, (1 << 256) - 2)
        # 3. r1 from the edge values, and r1 = 1 / edge: r1^-1, r1 and r1 r2 take them; 4. r2 from them
        pts = rand_points()
        for e in EDGES:
            good("r1=%x" % e, pts, e, rng.randrange(1, R))
            good("r1=1/%x" % e, pts, pow(e, -1, R), rng.randrange(1, R))
            good("r2=%x" % e, pts, rng.randrange(1, R), e)
        good("r1r2=lambda", pts, 3, LAMBDA * pow(3, -1, R) % R)
        # 5. points at infinity
        for name, sel in (("A=O", (0,)), ("B=O", (1,)), ("C=O", (2,)), ("ABC=O", (0, 1, 2))):
            p = list(rand_points())
            for s in sel:
                p[s] = None
            good(name, tuple(p), rng.randrange(1, R), rng.randrange(1, R))
        # 6 - 9. equal and opposite summands
        a, c0 = rng.randrange(1, R), rng.randrange(1, R)
        r1, r2 = rng.randrange(1, R), rng.randrange(1, R)
        A = E.mul(E.G1, a)
        B = E.g2_mul(E.G2, rng.randrange(1, R))
        good("B=r2.delta", (A, E.g2_mul(self.delta2, r2), E.mul(E.G1, c0)), r1, r2)
        good("B=-r2.delta", (A, E.g2_neg(E.g2_mul(self.delta2, r2)), E.mul(E.G1, c0)), r1, r2)
        assert not cases[-1].want[12:36].any()
        good("C=r2.A", (A, B, E.mul(A, r2)), r1, r2)
        good("C=-r2.A", (A, B, E.neg(E.mul(A, r2))), r1, r2)
        assert not cases[-1].want[36:].any()
        # 10. zero factors
        pts = rand_points()
        for name, f1, f2 in (("r1=0", 0, 5), ("r1=r", R, 5), ("r1=2r", 2 * R, 5), ("r2=0", 5, 0), ("r2=r", 5, R), ("r2=2r", 5, 2 * R)):
            cases.append(Case(name, proof_limbs(pts), f1, f2, ZERO_FACTOR, zeros))
        # 11. malformed proofs: refused whatever the flag (non-canonical, off the curve), or refused unless vouched for (outside the subgroup)
        base = proof_limbs(pts)
        f1, f2 = rng.randrange(1, R), rng.randrange(1, R)
        for name, at in (("A.x+q", 0), ("B.y.c1+q", 30), ("C.y+q", 42)):
            p = base.copy()
            p[at:at + 6] = _plus_q(p[at:at + 6])
            cases.append(Case(name, p, f1, f2, -1, zeros))
        cases.append(Case("A-off-curve", proof_limbs(((pts[0][0], (pts[0][1] + 1) % Q), pts[1], pts[2])), f1, f2, -1, zeros))
        cases.append(Case("B-off-curve", proof_limbs((pts[0], (pts[1][0], ((pts[1][1][0] + 1) % Q, pts[1][1][1])), pts[2])), f1, f2, -1, zeros))
        cases.append(Case("A-stray", proof_limbs((_stray(rng), pts[1], pts[2])), f1, f2, -1, zeros, 0, UNSPECIFIED))
        cases.append(Case("C-stray", proof_limbs((pts[0], pts[1], _stray(rng))), f1, f2, -1, zeros, 0, UNSPECIFIED))
        cases.append(Case("B-twist", proof_limbs((pts[0], _twist_point(rng), pts[2])), f1, f2, -1, zeros, 0, UNSPECIFIED))
        cases.append(Case("A-stray,r1=0", proof_limbs((_stray(rng), pts[1], pts[2])), 0, f2, -1, zeros, ZERO_FACTOR, zeros))
        self.cases = cases

    def proofs(self):
        return np.stack([c.proof for c in self.cases])

    def factors(self):
        return np.stack([c.factors for c in self.cases])

    def vk_dict(self):
        k = self.key
        return {"alpha_g1": E.mul(E.G1, k.alpha), "beta_g2": E.g2_mul(E.G2, k.beta), "gamma_g2": E.g2_mul(E.G2, k.gamma), "delta_g2": self.delta2,
                "gamma_abc_g1": [E.from_limbs(row) for row in k.gamma_abc]}


_CASES = None


def build(oracle):
    global _CASES
    if _CASES is None:
        _CASES = Cases(oracle)
    return _CASES


def check(cases, out, status, vouched):
    """out, status of the whole list in order against what is expected under the flag value"""
    out = np.asarray(out).view(np.uint64).reshape(-1, 48)
    for i, c in enumerate(cases.cases):
        st, want = (c.status_vouched, c.want_vouched) if vouched else (c.status, c.want)
        assert int(status[i]) == st, (c.name, vouched, int(status[i]))
        if isinstance(want, str):
            continue
        assert out[i].tolist() == want.tolist(), (c.name, vouched)
