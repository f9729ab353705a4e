"""Inputs with known verdicts for the Falcon verification entry points (frw_falcon_verify*), and the CPU side they are held to: a
numpy negacyclic product in int64, the two centring rules, and triples (sig, pk, hm) built to land on a chosen squared norm.  Shared by
tests/test_falcon_verify_rules.py (the oracle's circuit and the specification's sum on these triples, no GPU) and
tests/test_gpu_falcon_verify.py (the device on the same triples)."""
import math

import numpy as np

Q = 12289
BETA2 = {9: 34034726, 10: 70265242}
RULE_CIRCUIT, RULE_SPEC = 0, 1


def negacyclic(a, b):
    """a * b mod (x^N + 1, q), rows of int64; exact: the products stay below 2^38"""
    a, b = np.atleast_2d(np.asarray(a, dtype=np.int64)), np.atleast_2d(np.asarray(b, dtype=np.int64))
    n = a.shape[1]
    out = np.empty_like(a)
    for k in range(a.shape[0]):
        full = np.convolve(a[k], b[k])
        lo, hi = full[:n].copy(), full[n:]
        lo[:n - 1] -= hi
        out[k] = lo % Q
    return out


def v_of(sig, pk, hm):
    """v = hm - sig * pk, coefficients in [0, q)"""
    return (np.atleast_2d(np.asarray(hm, dtype=np.int64)) - negacyclic(sig, pk)) % Q


def centre(a, rule):
    """|centred representative| of a in [0, q): the circuits count a = 6144 as 6145 (is_less_than_6144), the specification as 6144"""
    a = np.asarray(a, dtype=np.int64)
    keep = a < 6144 if rule == RULE_CIRCUIT else a <= 6144
    return np.where(keep, a, Q - a)


def norms(sig, pk, hm, rule):
    """squared norm of v || sig per row, int64"""
    v = v_of(sig, pk, hm)
    s = np.atleast_2d(np.asarray(sig, dtype=np.int64))
    return (centre(v, rule) ** 2).sum(axis=1) + (centre(s, rule) ** 2).sum(axis=1)


def verdicts(nrm, logn, rule):
    """FRW_ST_OK / FRW_ST_NORM_BOUND per norm"""
    nrm = np.asarray(nrm, dtype=np.int64)
    refused = nrm >= BETA2[logn] if rule == RULE_CIRCUIT else nrm > BETA2[logn]
    return np.where(refused, 2, 0).astype(np.int32)


def four_squares(target):
    """a >= b >= c >= d >= 1, all below 6144, a^2 + b^2 + c^2 + d^2 = target (the largest such a first)"""
    for a in range(min(6143, math.isqrt(target)), 0, -1):
        ra = target - a * a
        for b in range(min(a, math.isqrt(ra)), 0, -1):
            rb = ra - b * b
            if rb > 2 * b * b:
                break
            for c in range(min(b, math.isqrt(rb)), 0, -1):
                d2 = rb - c * c
                d = math.isqrt(d2)
                if d > c:
                    break
                if d >= 1 and d * d == d2:
                    return a, b, c, d
    raise ValueError("no decomposition of %d" % target)


def sparse_triple(logn, pk, target, extra_v=None):
    """(sig, hm) for the given pk: sig has two non-zero coefficients and v two (one at index N - 1), signs mixed, their squares adding
    up to `target`; extra_v: {index: value} put into v besides.  hm = v + sig * pk."""
    n = 1 << logn
    a, b, c, d = four_squares(target)
    sig, v = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    sig[3], sig[n - 2] = a, Q - c                      # + a, - c
    v[0], v[n - 1] = Q - b, d                          # - b, + d
    for k, x in (extra_v or {}).items():
        assert v[k] == 0
        v[k] = x
    hm = (v + negacyclic(sig, pk)[0]) % Q
    return sig.astype(np.uint16), hm.astype(np.uint16)


def bound_triples(logn, pk3):
    """three triples on pk3[0..2] with norms beta^2 - 1, beta^2, beta^2 + 1 -> (sig, pk, hm) uint16[3, N], the norms"""
    want = [BETA2[logn] + k for k in (-1, 0, 1)]
    made = [sparse_triple(logn, pk3[k], want[k]) for k in range(3)]
    return np.stack([m[0] for m in made]), np.asarray(pk3, dtype=np.uint16), np.stack([m[1] for m in made]), want


def coeff_6144_triple(logn, pk):
    """v[5] = 6144.  Falcon-1024: the rest adds up to beta^2 - 6144^2 - 1, so the specification's sum is beta^2 - 1 and the circuits'
    beta^2 + 12288.  Falcon-512: 6144^2 alone is over the bound; the rest is 1,000,000."""
    rest = BETA2[logn] - 6144 * 6144 - 1 if logn == 10 else 1000000
    sig, hm = sparse_triple(logn, pk, rest, extra_v={5: 6144})
    return sig[None], np.asarray(pk, dtype=np.uint16)[None], hm[None], rest
