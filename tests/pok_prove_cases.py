"""Inputs for the prover from bytes (tests/test_gpu_pok_prove.py): encoded (public key, message, signature) triples with known verdicts
and the blinding factors that go with them.

    genuine(logn, count)   the Falcon triples of tests/golden/falcon_signed.json first (two per parameter set), then more signed here
                           with oracle/falcon_sign.py from the first fixture key's seed, as tests/test_gpu_falcon_verify.py does
    bad_header(triple)     the signature's header byte flipped                                   -> FRW_ST_DECODE
    bad_key(triple)        the key's first coefficient set to q = 12289                         -> FRW_ST_DECODE
    at_the_bound(logn)     a triple in BYTES whose squared norm under the circuits' rule is exactly beta^2 -> FRW_ST_NORM_BOUND.  Built the
                           way tests/falcon_verify_cases.py builds its coefficient triples (a sparse sig and a sparse v whose squares
                           add up to the target), except that from bytes hm is SHAKE256's, so the free polynomial is the public key:
                           pk = (hm - v) / sig in Z_q[x] / (x^N + 1), through a number-theoretic transform in numpy.
"""
import functools
import json
import os
import random

import numpy as np

import falcon_verify_cases as FV
from oracle import falcon_codec as FC
from oracle import falcon_sign as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = FV.Q
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
OK, COEFF_RANGE, NORM_BOUND, DECODE = 0, 1, 2, 3


def golden(logn):
    with open(os.path.join(ROOT, "tests", "golden", "falcon_signed.json")) as f:
        return [c for c in json.load(f)["cases"] if c["logn"] == logn]


@functools.lru_cache(maxsize=None)
def genuine(logn, count):
    """`count` genuine (pk_bytes, msg, sig_bytes), all different"""
    cases = golden(logn)
    out = [tuple(bytes.fromhex(c[k]) for k in ("pk_bytes", "msg", "sig_bytes")) for c in cases[:count]]
    if len(out) < count:
        seed = bytes.fromhex(cases[0]["key_seed"])
        sk = S.keygen(logn, seed)
        pkb = sk.public_key_bytes()
        assert pkb.hex() == cases[0]["pk_bytes"]
        for k in range(count - len(out)):
            msg = b"pok prove %d / %d" % (k, logn) + bytes(range(k))
            sgb = S.sign(sk, msg, seed + b"pok" + bytes([k]))
            assert S.verify(pkb, msg, sgb, logn) and len(sgb) == FC.SIG_LEN[logn]
            out.append((pkb, msg, sgb))
    return tuple(out)


def bad_header(triple):
    pkb, msg, sgb = triple
    return pkb, msg, bytes([sgb[0] ^ 1]) + sgb[1:]


def bad_key(triple):
    pkb, msg, sgb = triple
    return pkb[:1] + bytes([12289 >> 6, (12289 & 63) << 2 | (pkb[2] & 3)]) + pkb[3:], msg, sgb


def _ntt_matrix(logn):
    """V[j, k] = psi^((2 j + 1) k) mod q, psi a primitive 2N-th root of unity (7 has order 2048 mod 12289): a(x) -> its values at the
    roots of x^N + 1"""
    n = 1 << logn
    psi = pow(7, 2048 // (2 * n), Q)
    e = (np.outer(2 * np.arange(n) + 1, np.arange(n)) % (2 * n)).astype(np.int64)
    table = np.array([pow(psi, i, Q) for i in range(2 * n)], dtype=np.int64)
    return table[e], psi


@functools.lru_cache(maxsize=None)
def at_the_bound(logn):
    n = 1 << logn
    nonce = bytes((11 * i + logn) & 255 for i in range(FC.NONCE_LEN))
    msg = b"exactly at the bound"
    hm = np.array(FC.hash_to_point(nonce, msg, logn), dtype=np.int64)
    V, psi = _ntt_matrix(logn)
    for s0, s1 in ((100, -37), (101, -37), (100, -41), (97, -45)):
        signed = [0] * n
        signed[3], signed[n - 2] = s0, s1
        sig = np.array([x % Q for x in signed], dtype=np.int64)
        sig_hat = V @ sig % Q
        if (sig_hat == 0).any():
            continue                                            # not invertible: the next pair
        a, b, c, d = FV.four_squares(FV.BETA2[logn] - s0 * s0 - s1 * s1)
        v = np.zeros(n, dtype=np.int64)
        v[0], v[7], v[n // 2], v[n - 1] = Q - a, b, Q - c, d
        inv = np.array([pow(int(x), Q - 2, Q) for x in sig_hat], dtype=np.int64)
        pk_hat = (V @ ((hm - v) % Q) % Q) * inv % Q
        # the inverse transform: pk[k] = N^-1 sum_j pk_hat[j] psi^(-(2 j + 1) k)
        Vinv = np.array([pow(int(x), Q - 2, Q) for x in V.reshape(-1)], dtype=np.int64).reshape(n, n).T
        pk = Vinv @ pk_hat % Q * pow(n, Q - 2, Q) % Q
        assert (FV.v_of(sig, pk, hm)[0] == v).all()
        assert int(FV.norms(sig, pk, hm, FV.RULE_CIRCUIT)[0]) == FV.BETA2[logn]
        pkb = FC.modq_encode([int(x) for x in pk], logn)
        sgb = FC.comp_encode(signed, logn, nonce)
        assert FC.comp_decode(sgb, logn) == (nonce, [int(x) for x in sig]) and FC.modq_decode(pkb, logn) == [int(x) for x in pk]
        return pkb, msg, sgb
    raise AssertionError("no invertible sparse signature")


def blinding(tag):
    """(r, s) for an input, from a tag: the same input carries the same factors wherever it stands in a batch -> uint64[2, 4]"""
    rng = random.Random("pok prove rs %r" % (tag,))
    return np.frombuffer(b"".join(rng.randrange(R).to_bytes(32, "little") for _ in range(2)), dtype=np.uint64).reshape(2, 4).copy()
