"""The scalar side of the multi-scalar multiplications (falcon-r1cs_amd/csrc/frw_digits.h: scalar_canonical, scalar_is_one, signed_digits),
compiled for the host through the test-only shim (tests/cpp/hip_host) with the address and undefined-behaviour sanitizers and checked
against Python integers: the signed digits of every window width in use -- sixteen of 16 bits, thirty-two of 8, thirteen of 20 -- from
canonical and from Montgomery scalars, at the values where a digit is exactly half the window, where carries run to the top, and above r."""
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
WIDTHS = [(8, 32), (16, 16), (20, 13)]


def _scalars():
    rng = random.Random(2900)
    return ([0, 1, 2, R - 1, R, R + 5, 2 * R + 7, (1 << 256) - 1, (1 << 255) - 19,
             0x8000, 0x80, 0x7f81, 0x80000, (1 << 255) - (1 << 19) + 1,
             int("0001" * 16, 16), int("01" * 32, 16)]                   # (the repeated-digit vectors of tests/test_gpu_msm.py)
            + [rng.randrange(R) for _ in range(2000)])


def _digits(v, c, w):
    """tests/test_gpu_aggregate.py::_digits8 for any width: a window above 2^(c-1) borrows from the next, the top one takes the last carry"""
    out, carry = [], 0
    for j in range(w):
        d = ((v >> (c * j)) & ((1 << c) - 1)) + carry
        carry = 0
        if j < w - 1 and d > 1 << (c - 1):
            d -= 1 << c
            carry = 1
        out.append(d)
    return out


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(HERE, "cpp", "build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "test_digits")
    src = os.path.join(HERE, "cpp", "test_digits.cpp")
    hdrs = [os.path.join(ROOT, "falcon-r1cs_amd", "csrc", h) for h in ("frw_digits.h", "frw_fr29.h", "frw_fr.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas",
                               "-I", os.path.join(HERE, "cpp", "hip_host"), "-I", os.path.join(ROOT, "falcon-r1cs_amd", "csrc"), "-o", exe, src])

    def run(c, montgomery, values):
        text = "".join("%d %d %x\n" % (c, montgomery, v) for v in values)
        res = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120, check=True).stdout.split("\n")
        rows = [[int(x) for x in l.split()] for l in res if l]
        assert len(rows) == len(values)
        return [(row[0] == 1, row[1:]) for row in rows]
    return run


@pytest.mark.parametrize("montgomery", [0, 1], ids=["canonical", "montgomery"])
@pytest.mark.parametrize("c,w", WIDTHS, ids=["8bit", "16bit", "20bit"])
def test_signed_digits_equal_python_integers(harness, c, w, montgomery):
    values = _scalars()
    given = [v * (1 << 256) % R for v in values] if montgomery else values
    half = 1 << (c - 1)
    for v, (one, d) in zip(values, harness(c, montgomery, given)):
        k = v % R
        assert d == _digits(k, c, w), hex(v)
        assert sum(dj << (c * j) for j, dj in enumerate(d)) == k, hex(v)
        assert all(-half + 1 <= dj <= half for dj in d) and 0 <= d[-1] <= half, hex(v)
        assert one == (k == 1), hex(v)
