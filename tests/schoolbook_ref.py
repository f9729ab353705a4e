"""Shared helpers of the schoolbook-circuit tests: the ORACLE's FalconSchoolBookVerificationCircuit
(oracle/falcon_gadgets.py run on oracle/ark_sim.py) as the expected witness, instance vector and matrices, the fixture
triples, and the committed digests of tests/golden/schoolbook_{512,1024}.json (written by tests/golden/make_schoolbook.py).
Nothing here touches the product."""
import functools
import hashlib
import json
import os
import random

import numpy as np

import frw_testlib as T
from oracle import falcon_gadgets as G

P = G.P_BLS12_381_FR
Q = G.MODULUS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CIRCUIT_SCHOOLBOOK = 2
# fixture seeds: two triples per parameter set (the second one replaces a slot of the ragged batches)
SEEDS = {9: (2901, 2902), 10: (3001, 3002)}


def counts(logn):
    """README.md:45,56 of the reference: (I, W, C) of FalconSchoolBookVerificationCircuit."""
    n, nb = 1 << logn, 50 if logn == 9 else 52
    return 2 * n + 1, n * n + 99 * n + nb, n * n + 105 * n + nb + 2


def triple(logn, seed):
    sig, pk, hm, _ = T.random_triple(logn, random.Random(seed))
    return sig, pk, hm


def oracle_cs(sig, pk, hm, logn, strict=False):
    cs = G.ConstraintSystem()
    G.FalconSchoolBookVerificationCircuit([int(x) for x in sig], [int(x) for x in pk], [int(x) for x in hm], logn).generate_constraints(cs, strict)
    return cs


@functools.lru_cache(maxsize=4)
def fixture_cs(logn, which=0):
    """The oracle's constraint system of fixture triple `which` (computed once per session and shared; do not modify)."""
    return oracle_cs(*triple(logn, SEEDS[logn][which]), logn, strict=True)


def encoded(cs, montgomery):
    """(witness bytes, instance bytes) of the oracle's assignment in the product's two encodings."""
    return G.encode_elements(cs.witness_assignment, montgomery), G.encode_elements(cs.instance_assignment, montgomery)


def tail_counts(cs, logn):
    """How many columns end in [0, 1, 1, (-q)^-1, 0] (hm[i] < c) and in [1, q^-1, 0, 1, 0] (hm[i] >= c)."""
    n = 1 << logn
    qinv, nqinv = pow(Q, -1, P), pow(P - Q, -1, P)
    lt = ge = 0
    for i in range(n):
        tail = cs.witness_assignment[29 * n + i * (n + 34) + n + 29:29 * n + (i + 1) * (n + 34)]
        if tail == [0, 1, 1, nqinv, 0]:
            lt += 1
        elif tail == [1, qinv, 0, 1, 0]:
            ge += 1
    return lt, ge


def sha(b):
    return hashlib.sha256(b).hexdigest()


def golden(logn):
    return json.load(open(os.path.join(GOLDEN, "schoolbook_%d.json" % (1 << logn))))


def golden_triple(g, which):
    t = g["triples"][which]
    return tuple(np.frombuffer(bytes.fromhex(t[k]), dtype=np.uint16).copy() for k in ("sig", "pk", "hm"))
