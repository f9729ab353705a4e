"""Re-randomising proofs (frw_groth16_rerandomize and its device forms) where no GPU is needed: the symbols exist in the library, the
header, the ctypes table and the Rust declarations; every refusal the header lists; batch = 0; FRW_E_NO_DEVICE for the device calls
on a machine without one; the workspace sizes against falcon-r1cs_amd/csrc/frw_layout.h rerand_layout (compiled for the host through
the test-only shim); the factors' arithmetic of frw_rerand.h against Python integers; and the stand-alone program of
tools/sanitize_cpu.sh under AddressSanitizer and UndefinedBehaviorSanitizer."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import falcon_r1cs_amd as frw
import frw_testlib as T
from oracle import bls12_381 as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("frw_groth16_rerandomize", "frw_groth16_rerandomize_workspace_bytes", "frw_groth16_rerandomize_dev", "frw_groth16_rerandomize_wire_dev")
OK, INVALID, NO_DEVICE = 0, -1, -2
R = E.R
LAMBDA = 0xac45a4010001a40200000000ffffffff
SRC = os.path.join(HERE, "cpp", "test_rerand_host.cpp")
INCLUDES = ["-I", os.path.join(HERE, "cpp", "hip_host"), "-I", os.path.join(ROOT, "falcon-r1cs_amd", "csrc")]


def test_the_new_symbols_are_exported_and_declared():
    frw.load_library()                       # (first: it maps torch's HIP runtime before the library's own, see _lib.py)
    lib = C.CDLL(frw.lib_path())
    header = open(os.path.join(ROOT, "include", "frw.h")).read()
    rust = open(os.path.join(ROOT, "rust", "frw-sys", "src", "lib.rs")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in frw._lib.PROTOTYPES, name
        assert "pub fn %s(" % name in rust, name
    assert re.search(r"#define FRW_RERAND_ZERO_FACTOR \(-2\)", header) and "pub const FRW_RERAND_ZERO_FACTOR: c_int = -2;" in rust
    assert frw.engine.RERAND_ZERO_FACTOR == -2
    for method in ("rerandomize", "rerandomize_dev", "rerandomize_wire_dev", "rerandomize_workspace_bytes"):
        assert callable(getattr(frw.Groth16Verifier, method))
    # what the header must say: in place, the vouching flag's caveat, freshness
    section = header[header.index("re-randomising proofs"):header.index("#define FRW_RERAND_ZERO_FACTOR")]
    for phrase in ("read whole before any of it is written", "unspecified", "memory-safe and deterministic", "FRESH"):
        assert phrase in section, phrase


@pytest.fixture(scope="module")
def host_key(oracle):
    import rerandomize_cases as RC
    cs = RC.build(oracle)
    ver = frw.Groth16Verifier(cs.key.limbs())
    yield cs, ver
    ver.close()


@pytest.fixture(scope="module")
def layout_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rerand") / "libtest_rerand.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-fno-strict-aliasing"] + INCLUDES + ["-o", so, SRC])
    lib = C.CDLL(so)
    lib.t_rerand_layout.restype = C.c_uint64
    lib.t_rerand_layout.argtypes = [C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
    lib.t_rerand_factors.restype = C.c_int
    lib.t_rerand_factors.argtypes = [C.c_void_p, C.c_void_p]
    return lib


def _args(ver, **kw):
    """valid-looking arguments of frw_groth16_rerandomize_dev (pointers into host memory: no check below dereferences them)"""
    buf = (C.c_uint64 * 512)()
    p = C.c_void_p((C.addressof(buf) + 255) & ~255)
    a = dict(vk=ver._h, batch=1, proofs=p, factors=p, flags=0, out=p, status=p, ws=p, ws_bytes=1 << 20, stream=None, keep=buf)
    a.update(kw)
    return a


def _dev(lib, a):
    return lib.frw_groth16_rerandomize_dev(a["vk"], a["batch"], a["proofs"], a["factors"], a["flags"], a["out"], a["status"], a["ws"], a["ws_bytes"], a["stream"])


def _wire(lib, a, mode=0):
    return lib.frw_groth16_rerandomize_wire_dev(a["vk"], a["batch"], a["proofs"], mode, a["factors"], a["flags"], a["out"], a["status"], a["ws"],
                                                a["ws_bytes"], a["stream"])


def test_refusals_of_the_device_calls(host_key):
    _, ver = host_key
    lib = frw.load_library()
    for call in (_dev, _wire):
        for null in ("vk", "proofs", "factors", "out", "status", "ws"):
            assert call(lib, _args(ver, **{null: None})) == INVALID, (call.__name__, null)
        for flags in (2, 4, 3, -1, 1 << 16):
            assert call(lib, _args(ver, flags=flags)) == INVALID, flags
        a = _args(ver)
        assert call(lib, _args(ver, ws=C.c_void_p(a["ws"].value + 8), keep2=a)) == INVALID          # misaligned
        # batch = 0: a no-op that returns before the handle, or anything else, is looked at
        assert call(lib, _args(ver, batch=0, vk=None, proofs=None, flags=99, ws=None)) == OK
    for mode in (-1, 2, 7):
        assert _wire(lib, _args(ver), mode) == INVALID, mode


def test_no_device_and_keys_without_a_device_part(host_key):
    """On a machine without a device the device calls say so (no host fallback); where there is one, a host key is refused: only
    frw_groth16_vk_load_dev / _load_wire_dev put delta_g2 on the device."""
    _, ver = host_key
    lib = frw.load_library()
    want = NO_DEVICE if lib.frw_device_count() <= 0 else INVALID
    for flags in (0, 1):
        assert _dev(lib, _args(ver, flags=flags)) == want
        for mode in (0, 1):
            assert _wire(lib, _args(ver, flags=flags), mode) == want


def test_refusals_of_the_host_function(host_key):
    cs, ver = host_key
    lib = frw.load_library()
    p = cs.proofs()[:1].copy()
    f = cs.factors()[:1].copy()
    out = np.zeros((1, 48), dtype=np.uint64)
    st = np.zeros(1, dtype=np.int32)
    v = lambda a: a.ctypes.data_as(C.c_void_p)
    good = [ver._h, 1, v(p), v(f), 0, v(out), v(st)]
    assert lib.frw_groth16_rerandomize(*good) == OK and st[0] == 0
    for i in (0, 2, 3, 5, 6):
        bad = list(good)
        bad[i] = None
        assert lib.frw_groth16_rerandomize(*bad) == INVALID, i
    for flags in (2, 3, 4, -1):
        bad = list(good)
        bad[4] = flags
        assert lib.frw_groth16_rerandomize(*bad) == INVALID, flags
    assert lib.frw_groth16_rerandomize(None, 0, None, None, 99, None, None) == OK


def test_workspace_sizes_are_the_layouts(host_key, layout_lib):
    _, ver = host_key
    out = (C.c_uint64 * 12)()
    for wire_mode, wire in ((None, 0), (frw.engine.WIRE_COMPRESSED, 1), (frw.engine.WIRE_UNCOMPRESSED, 1)):
        last = 0
        for k in (1, 2, 3, 7, 64, 65, 1030, 16384):
            size = ver.rerandomize_workspace_bytes(k, wire_mode)
            assert size == layout_lib.t_rerand_layout(k, wire, out) and size % 16 == 0
            assert size > last                                                       # monotone in the proofs in flight
            last = size
            pieces = [(out[2 * i], out[2 * i + 1]) for i in range(6 if wire else 3)]
            end = 0
            for off, length in pieces:                                               # in order, 16-byte aligned, disjoint, inside
                assert off % 16 == 0 and off >= end and length > 0
                end = off + length
            assert end <= size
        per = 128 + 2 * 240 + 464 + (384 + 4 + 4 if wire else 0)
        assert ver.rerandomize_workspace_bytes(16, wire_mode) == 16 * per                 # (every piece a multiple of 16 at k = 16)
    assert ver.rerandomize_workspace_bytes(0) == 0
    lib = frw.load_library()
    assert lib.frw_groth16_rerandomize_workspace_bytes(None, 4, -1) == 0
    for mode in (-2, 2, 5):
        assert lib.frw_groth16_rerandomize_workspace_bytes(ver._h, 4, mode) == 0


def test_the_factors_arithmetic_against_python_integers(layout_lib):
    """frw_rerand.h factors_prepare: reduction modulo r, the zero test, r1^-1 and r2 split by lambda, r1, r1 r2"""
    rng = random.Random(5)
    edges = [1, 2, 3, LAMBDA - 1, LAMBDA, LAMBDA + 1, 2 * LAMBDA, 1 << 127, (1 << 128) - 1, R - 2, R - 1, R + 1, 2 * R + 1, (1 << 256) - 1, 1 << 255]
    pairs = [(a, b) for a in edges for b in (edges[0], edges[4], edges[-2])] + [(b, a) for a in edges for b in (5, R - 1)]
    pairs += [(pow(e, -1, R), 7) for e in edges[:11]] + [(rng.randrange(1 << 256), rng.randrange(1 << 256)) for _ in range(200)]
    out = np.zeros(16, dtype=np.uint64)
    for r1, r2 in pairs:
        f = T.ints_to_limbs([r1, r2])
        assert layout_lib.t_rerand_factors(f.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 0
        w = [int(x) for x in out]
        val = lambda i, n: sum(w[i + j] << (64 * j) for j in range(n))
        inv, b = pow(r1 % R, -1, R), r2 % R
        assert (val(0, 2), val(2, 2)) == (inv % LAMBDA, inv // LAMBDA), hex(r1)
        assert (val(4, 2), val(6, 2)) == (b % LAMBDA, b // LAMBDA), hex(r2)
        assert val(8, 4) == r1 % R and val(12, 4) == (r1 % R) * b % R
    for r1, r2 in ((0, 5), (R, 5), (2 * R, 5), (5, 0), (5, R), (5, 2 * R), (0, 0)):
        f = T.ints_to_limbs([r1, r2])
        assert layout_lib.t_rerand_factors(f.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == -2


def test_the_stand_alone_program_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "rerand_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wno-unknown-pragmas", "-fno-strict-aliasing"] + INCLUDES + ["-o", exe, SRC])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert res.returncode == 0, res.stdout
    assert res.stdout.strip().endswith("rerandomize host path: clean"), res.stdout
    script = open(os.path.join(ROOT, "tools", "sanitize_cpu.sh")).read()
    assert "tests/cpp/test_rerand_host.cpp" in script
