"""The reference of the factor draw (falcon-r1cs_amd/csrc/frw_drbg.h), in hashlib and Python integers:
    x_j = int_le(SHAKE256("FRW-FR-DRAW-001" || tag || seed || le64(counter) || le64(j))[:64]) mod r
What tests/test_drbg_host.py, tests/test_drbg_abi.py and tests/test_gpu_drbg.py compare with, bit for bit."""
import hashlib

import numpy as np

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
TWO256_MOD_R = 0x1824b159acc5056f998c4fefecbc4ff55884b7fa0003480200000001fffffffe
DOMAIN = b"FRW-FR-DRAW-001"
BLINDING, RERANDOMIZE = 1, 2
SEED = bytes(range(32))
KNOWN_ANSWER = 0x19aaf15ed9ea1d6ca2f5819bb24ee21b7f0353193eaf03042c8235cdaabe84f5      # SEED, counter 0, tag 1, j 0

assert (1 << 256) % R == TWO256_MOD_R and len(DOMAIN) == 15


def wide(seed, counter, tag, j):
    """the 512-bit integer before the reduction"""
    assert len(seed) == 32 and 0 <= tag < 256 and 0 <= counter < 1 << 64 and 0 <= j < 1 << 64
    msg = DOMAIN + bytes([tag]) + bytes(seed) + counter.to_bytes(8, "little") + j.to_bytes(8, "little")
    return int.from_bytes(hashlib.shake_256(msg).digest(64), "little")


def scalar(seed, counter, tag, j):
    return wide(seed, counter, tag, j) % R


def scalars(seed, counter, tag, count):
    return [scalar(seed, counter, tag, j) for j in range(count)]


def limbs(values):
    """Python integers below 2^256 -> uint64[len, 4], little-endian words"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint64).reshape(-1, 4).copy()


def draw(seed, counter, tag, count):
    """what frw_fr_draw writes: uint64[count, 4]"""
    return limbs(scalars(seed, counter, tag, count))


def factors(seed, counter, tag, batch):
    """what a composed call leaves in d_rs / d_factors: uint64[batch, 2, 4], slot i = elements 2 i and 2 i + 1"""
    return draw(seed, counter, tag, 2 * batch).reshape(batch, 2, 4)


assert scalar(SEED, 0, 1, 0) == KNOWN_ANSWER
