"""The per-item functions of Falcon's encodings (falcon-r1cs_amd/csrc/frw_codec.h: hash_to_point_one, public_key_coeff with its two
refusal tests, decode_signature_one), compiled for the host through the test-only shim (tests/cpp/hip_host) and driven through the whole
catalogue of tests/falcon_codec_cases.py against oracle/falcon_codec.py: the comparison tests/test_gpu_codec.py makes on the device, on
every machine.  All of it exact: verdicts, uint16 coefficients, nonce bytes.

The device cannot show a read past sig_len, past a key or past a message's end.  test_sanitized_standalone_run does: it dumps the
catalogue to a temporary file, compiles tests/cpp/codec_sanitize_main.cpp with -fsanitize=address,undefined and runs it as a child
process; every input there lives in a heap buffer of exactly its length.

FRW_TEST_CODEC_CSRC=<dir> takes frw_codec.h from <dir> instead of the product's (built in a temporary directory): how a deliberately
faulty copy of the header is shown to fail these tests."""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import falcon_codec_cases as CC
from oracle import falcon_codec as FC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "falcon-r1cs_amd", "csrc")
OVERRIDE = os.environ.get("FRW_TEST_CODEC_CSRC")
INCLUDES = ["-I", os.path.join(HERE, "cpp", "hip_host")] + (["-I", OVERRIDE] if OVERRIDE else []) + ["-I", CSRC]
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-function"]
ROW_SENTINEL, NONCE_SENTINEL, GUARD = 0xFFFF, 0xEE, 64


@pytest.fixture(scope="module")
def cat():
    return CC.catalogue()


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(HERE, "cpp", "test_codec.cpp")
    deps = [src] + [os.path.join(OVERRIDE or CSRC, "frw_codec.h"), os.path.join(CSRC, "frw_keccak.h"), os.path.join(HERE, "cpp", "hip_host", "hip", "hip_runtime.h")]
    if OVERRIDE:
        out = tempfile.mkdtemp(prefix="frw_codec_")
    else:
        out = os.path.join(HERE, "cpp", "build")
        os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libtest_codec.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC"] + FLAGS + INCLUDES + ["-o", so, src])
    lib = C.CDLL(so)
    lib.t_decode_signature.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.t_decode_public_key.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.t_hash_to_point.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.t_hash_to_point.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _in(data):
    return np.frombuffer(bytes(data) or b"\0", dtype=np.uint8).copy()


def decode_signature(lib, logn, data, want_nonce=True):
    """(accepted, the row, the nonce row or None); a row of N coefficients with GUARD sentinels behind it that must stay"""
    n = 1 << logn
    row = np.full(n + GUARD, ROW_SENTINEL, dtype=np.uint16)
    nonce = np.full(40 + GUARD, NONCE_SENTINEL, dtype=np.uint8)
    ok = lib.t_decode_signature(logn, _p(_in(data)), len(data), _p(row), _p(nonce) if want_nonce else None)
    assert (row[n:] == ROW_SENTINEL).all() and (nonce[40:] == NONCE_SENTINEL).all()
    assert want_nonce or (nonce == NONCE_SENTINEL).all()
    return bool(ok), row[:n], nonce[:40] if want_nonce else None


def check_signature(lib, logn, data, want, where):
    ok, row, nonce = decode_signature(lib, logn, data)
    ok2, row2, _ = decode_signature(lib, logn, data, want_nonce=False)
    assert ok == ok2 == (want is not None), where
    if want is not None:
        assert row.tolist() == want[1] and row2.tolist() == want[1], where
        assert nonce.tobytes() == want[0] == bytes(data[1:41]), where
    if not data or data[0] != 0x30 + logn:
        assert (nonce == NONCE_SENTINEL).all(), "%s: the nonce is copied out only behind the expected header" % where


@pytest.mark.parametrize("logn", CC.LOGNS)
def test_signatures_against_the_oracle(lib, cat, logn):
    seen = set()
    for c in cat.signatures(logn):
        check_signature(lib, logn, c.data, c.want, c.name)
        if c.twin is not None and c.twin not in seen:
            seen.add(c.twin)
            twin = FC.comp_decode(c.twin, logn)
            assert twin is not None
            check_signature(lib, logn, c.twin, twin, "the twin of " + c.name)
    # lengths the entry points refuse as arguments: no byte is read, nothing is written
    for sig_len in (0, 1, 40, 41):
        ok, row, nonce = decode_signature(lib, logn, (bytes([0x30 + logn]) + bytes(40))[:sig_len])
        assert not ok and (row == ROW_SENTINEL).all() and (nonce == NONCE_SENTINEL).all()


@pytest.mark.parametrize("logn", CC.LOGNS)
def test_public_keys_against_the_oracle(lib, cat, logn):
    n = 1 << logn
    for k in cat.keys[logn]:
        for data, want in ((k.data, k.want),) + (((k.twin, FC.modq_decode(k.twin, logn)),) if k.twin else ()):
            row = np.full(n + GUARD, ROW_SENTINEL, dtype=np.uint16)
            ok = lib.t_decode_public_key(logn, _p(_in(data)), _p(row))
            assert (row[n:] == ROW_SENTINEL).all()
            assert bool(ok) == (want is not None), k.name
            if want is not None:
                assert row[:n].tolist() == want, k.name


@pytest.mark.parametrize("logn", CC.LOGNS)
def test_hash_to_point_against_the_oracle(lib, cat, logn):
    n = 1 << logn

    def run(nonce, msg, o0, o1):
        row = np.full(n + GUARD, ROW_SENTINEL, dtype=np.uint16)
        lib.t_hash_to_point(logn, _p(_in(nonce)), _p(_in(msg)), o0, o1, _p(row))
        assert (row[n:] == ROW_SENTINEL).all()
        return row[:n].tolist()

    for h in cat.hashes[logn]:
        assert run(h.nonce, h.msg, 0, len(h.msg)) == h.want, h.name
        assert max(h.want) < CC.Q
    h = cat.hashes[logn][7]
    assert run(h.nonce, h.msg, 1 << 40, (1 << 40) + len(h.msg)) == h.want              # the offsets count, not where they start
    assert run(h.nonce, h.msg, 5, 3) == FC.hash_to_point(h.nonce, b"", logn)            # decreasing offsets: an empty message


def write_dump(cat, path):
    """the catalogue as tests/cpp/codec_sanitize_main.cpp reads it (the format is described there) -> the number of cases"""
    records = []

    def record(kind, logn, data, row, nonce=b""):
        records.append(struct.pack("<BBBBI", kind, logn, row is not None, 0, len(data)) + nonce + bytes(data)
                       + (np.asarray(row, dtype="<u2").tobytes() if row is not None else b""))

    for logn in CC.LOGNS:
        for c in cat.signatures(logn):
            record(0, logn, c.data, c.want[1] if c.want else None)
        for k in cat.keys[logn]:
            record(1, logn, k.data, k.want)
        for h in cat.hashes[logn]:
            record(2, logn, h.msg, h.want, h.nonce)
    with open(path, "wb") as f:
        f.write(b"FRWCODEC" + struct.pack("<I", len(records)) + b"".join(records))
    return len(records)


def test_sanitized_standalone_run(cat, tmp_path):
    dump, exe = str(tmp_path / "catalogue.bin"), str(tmp_path / "codec_sanitize")
    count = write_dump(cat, dump)
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"] + FLAGS + INCLUDES
                          + ["-o", exe, os.path.join(HERE, "cpp", "codec_sanitize_main.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    run = subprocess.run([exe, dump], capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    sizes = cat.sizes()
    want = tuple(sum(sizes[g][k] for g in CC.LOGNS for k in keys) for keys in (("well-formed", "refused", "mutants"), ("keys",), ("hashes",)))
    assert run.stdout.strip() == "%d signatures, %d keys, %d hashes: 0 mismatches" % want and sum(want) == count
