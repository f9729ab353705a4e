"""The run-time-field arithmetic of the witness kernels (falcon-r1cs_amd/csrc/frw_field.h), compiled for the host through the test-only
shim (tests/cpp/hip_host) with AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program, and checked against Python
integers: the constants derived from a modulus by shift-and-reduce, the one-round and five-round conversions at their edges, and the
refusals.  The same header serves frw_field_info, frw_expand_field_host and the ENC = 3 kernels."""
import os
import random
import re
import subprocess

import pytest

import field_cases as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "falcon-r1cs_amd", "csrc")


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(HERE, "cpp", "build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "test_field")
    src = os.path.join(HERE, "cpp", "test_field.cpp")
    hdr = os.path.join(CSRC, "frw_field.h")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in (src, hdr)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas",
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", os.path.join(HERE, "cpp", "hip_host"), "-I", CSRC, "-o", exe, src])

    def run(ops):
        text = "\n".join("%s %s" % (op, " ".join("%x" % v for v in args)) for op, *args in ops) + "\n"
        res = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr[-2000:]          # a sanitizer report ends the program with a non-zero status
        return [l.split() for l in res.stdout.split("\n") if l]
    return run


def test_constants_of_every_modulus(harness):
    names = list(F.MODULI)
    got = harness([("consts", F.MODULI[n]) for n in names])
    for n, g in zip(names, got):
        p, want = F.MODULI[n], F.consts(F.MODULI[n])
        assert g[0] == "ok", n
        one, k1, k5, r2, ninv, bits, pp = (int(v, 16) for v in g[1:])
        assert (one, k1, k5, r2, ninv, bits, pp) == (want["one"], want["k1"], want["k5"], want["r2"], want["ninv32"], want["bits"], p), n
    # the published limbs of ark-bn254's one, and the digit shortcut m = -T[0] that holds for BLS12-381 only among these
    assert F.limbs4(F.consts(F.BN254)["one"]) == list(F.BN254_ONE_LIMBS)
    assert F.consts(F.BN254)["ninv32"] == 0xEFFFFFFF and F.consts(F.BLS12_381)["ninv32"] == 0xFFFFFFFF
    assert F.consts(F.BLS12_377)["ninv32"] == 0xFFFFFFFF and F.consts(F.ED25519_L)["ninv32"] != 0xFFFFFFFF


def test_bls12_381_constants_equal_the_kernel_literals(harness):
    text = open(os.path.join(CSRC, "frw_kernels.hip")).read()

    def literal(name):
        words = re.search(r"#define %s\s+\{([^}]*)\}" % name, text).group(1)
        return sum(int(w.strip().rstrip("u"), 16) << (32 * i) for i, w in enumerate(words.split(",")))
    g = harness([("consts", F.BLS12_381)])[0]
    one, k1, k5, _, ninv, _, pp = (int(v, 16) for v in g[1:])
    assert (pp, one, k1, k5) == (literal("FRW_P32"), literal("FRW_R32"), literal("FRW_K1"), literal("FRW_K5"))
    assert ninv == 0xFFFFFFFF


def test_encodings_against_python_integers(harness):
    rng = random.Random(160)
    assert F.LADDER_MAX.bit_length() == 160
    ops = []
    for p in F.MODULI.values():
        for x in [0, 1, F.Q, (1 << 32) - 1] + [rng.getrandbits(32) for _ in range(40)]:
            ops.append(("u32", p, x))
        for x in [0, (1 << 160) - 1, F.LADDER_MAX, 1, (1 << 32) - 1, 1 << 32, 1 << 159] + [rng.getrandbits(160) for _ in range(40)] + \
                 [rng.getrandbits(rng.randrange(1, 161)) for _ in range(20)]:
            ops.append(("u160", p, x))
    for (op, p, x), g in zip(ops, harness(ops)):
        v = int(g[0], 16)
        assert v < p and v == F.mont(x, p), (op, hex(p), hex(x))


def test_inadmissible_moduli_are_refused(harness):
    names = list(F.REFUSED)
    got = harness([("consts", F.REFUSED[n]) for n in names] + [("u32", F.REFUSED[n], 5) for n in names] +
                  [("consts", (1 << 161) - 1), ("consts", (1 << 160) + 1), ("consts", (1 << 255) - 1), ("consts", (1 << 256) + 1)])
    assert [g[0] for g in got] == ["refused"] * (2 * len(names)) + ["ok", "ok", "ok", "refused"]
