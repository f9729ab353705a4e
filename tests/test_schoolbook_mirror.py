"""The schoolbook circuit in the C++ host mirror (falcon-r1cs_amd/csrc/host/frw_host.hpp), through
tests/cpp/test_schoolbook_mirror.cpp.  CPU: the mirror's own counters in setup mode reproduce the third row of the
reference's count table.  GPU: the reference's test_schoolbook_verification_r1cs (falcon_schoolbook.rs:141-169)
re-stated on it, every witness value coming from the HIP engine."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "build")
BIN = os.path.join(BUILD, "test_schoolbook_mirror")


@pytest.fixture(scope="module")
def mirror_bin():
    src = os.path.join(ROOT, "tests", "cpp", "test_schoolbook_mirror.cpp")
    hdr = os.path.join(ROOT, "falcon-r1cs_amd", "csrc", "host", "frw_host.hpp")
    lib = os.path.join(ROOT, "falcon-r1cs_amd", "libfrw.so")
    assert os.path.exists(lib), "libfrw.so not built; run __graft_entry__.build()"
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(p) for p in (src, hdr, lib)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", BIN, src,
                               "-L" + os.path.dirname(lib), "-lfrw", "-Wl,-rpath,$ORIGIN/../../../falcon-r1cs_amd"])
    return BIN


def test_mirror_counters_reproduce_the_published_row(mirror_bin):
    out = subprocess.run([mirror_bin, "structure"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all passed" in out.stdout, out.stdout + out.stderr
    for want in ("312882", "315956", "1150004", "1156150", "1025", "2049"):
        assert want in out.stdout, (want, out.stdout)


@pytest.mark.gpu
def test_reference_unit_test_on_the_engine(mirror_bin):
    out = subprocess.run([mirror_bin, "gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "all passed" in out.stdout and "FAILED" not in out.stdout, out.stdout + out.stderr
