"""The factor draw's one definition (falcon-r1cs_amd/csrc/frw_drbg.h: the message, the host's Keccak-f[1600], the 512-bit reduction over
frw_rerand.h's integers), compiled for the host through the test-only shim (tests/cpp/hip_host) with AddressSanitizer and
UndefinedBehaviorSanitizer as a stand-alone program, and checked bit for bit against hashlib and Python integers (tests/drbg_ref.py)."""
import os
import random
import subprocess

import pytest

import drbg_ref as D

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "falcon-r1cs_amd", "csrc")
R, M = D.R, (1 << 256) - 1


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(HERE, "cpp", "build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "test_drbg_host")
    src = os.path.join(HERE, "cpp", "test_drbg_host.cpp")
    hdrs = [os.path.join(CSRC, h) for h in ("frw_drbg.h", "frw_rerand.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", os.path.join(HERE, "cpp", "hip_host"), "-I", CSRC, "-o", exe, src])

    def run(ops):
        text = "\n".join("%s %s" % (op, " ".join(a if isinstance(a, str) else "%x" % a for a in args)) for op, *args in ops) + "\n"
        res = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr[-2000:]          # a sanitizer report ends the program with a non-zero status
        return [int(l, 16) for l in res.stdout.split("\n") if l]
    return run


def test_the_wide_reduction_against_python_integers(harness):
    rng = random.Random(512)
    edges = [0, R - 1, R, 2 * R - 1, 2 * R, M]
    pairs = [(lo, 0) for lo in edges] + [(0, hi) for hi in edges] + [(lo, hi) for lo in edges for hi in edges]
    pairs += [(M, R - 1), (M, M)]                                # hi = r - 1 with lo = 2^256 - 1; 2^512 - 1
    pairs += [(v & M, v >> 256) for v in (rng.getrandbits(512) for _ in range(200))]
    assert (M, R - 1) in pairs and (M, M) in pairs and len(pairs) >= 200 + 14
    got = harness([("reduce", lo, hi) for lo, hi in pairs])
    for (lo, hi), g in zip(pairs, got):
        assert g == (lo + (hi << 256)) % R, (hex(lo), hex(hi))


def test_the_derivation_against_hashlib(harness):
    """seed 00 .. 1f, tag 1, counter 0, j = 0 .. 63 -- among them each half of the 512 bits falls in [0, r), [r, 2r) and [2r, 2^256) at
    least four times, so every path of fr_reduce is taken on hashed inputs too -- and other counters, tags and indices"""
    for half in (lambda w: w & M, lambda w: w >> 256):
        where = [half(D.wide(D.SEED, 0, 1, j)) // R for j in range(64)]
        assert min(where.count(k) for k in (0, 1, 2)) >= 4
    seed = D.SEED.hex()
    cases = [(0, 1, j) for j in range(64)]
    cases += [(c, tag, j) for c in (1, 1 << 32, (1 << 64) - 1) for tag in (0, 2, 255) for j in (0, 1, (1 << 32) + 5, (1 << 64) - 1)]
    got = harness([("draw", seed, c, tag, j) for c, tag, j in cases])
    for (c, tag, j), g in zip(cases, got):
        assert g == D.scalar(D.SEED, c, tag, j) and g < R, (c, tag, j)
    other = bytes(random.Random(32).getrandbits(8) for _ in range(32))
    got = harness([("draw", other.hex(), 7, 2, j) for j in range(8)])
    assert got == D.scalars(other, 7, 2, 8)


def test_the_known_answer(harness):
    assert harness([("draw", D.SEED.hex(), 0, 1, 0)]) == [D.KNOWN_ANSWER]
    assert D.KNOWN_ANSWER == 0x19aaf15ed9ea1d6ca2f5819bb24ee21b7f0353193eaf03042c8235cdaabe84f5
