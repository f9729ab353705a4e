"""Drawing the factors (frw_fr_draw and the device forms) where no GPU is needed: frw_fr_draw through ctypes against hashlib
(tests/drbg_ref.py), its refusals, what it writes and what it leaves alone; the five symbols in the library, the header, the ctypes
table, the Rust declarations and the Python face; the device calls' refusals that come before any device is looked at."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import falcon_r1cs_amd as frw
import drbg_ref as D

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("frw_fr_draw", "frw_fr_draw_dev", "frw_groth16_prove_seeded_dev", "frw_groth16_rerandomize_seeded_dev",
       "frw_groth16_rerandomize_wire_seeded_dev")
OK, INVALID, NO_DEVICE = 0, -1, -2
GUARD = 0xA5A5A5A5A5A5A5A5


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _seed(seed=D.SEED):
    return np.frombuffer(seed, dtype=np.uint8).copy()


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
    assert re.search(r"#define FRW_DRAW_BLINDING\s+1\b", header) and re.search(r"#define FRW_DRAW_RERANDOMIZE\s+2\b", header)
    assert "pub const FRW_DRAW_BLINDING: c_int = 1;" in rust and "pub const FRW_DRAW_RERANDOMIZE: c_int = 2;" in rust
    assert (frw.DRAW_BLINDING, frw.DRAW_RERANDOMIZE) == (1, 2) == (D.BLINDING, D.RERANDOMIZE)
    assert callable(frw.fr_draw) and callable(frw.fr_draw_dev) and callable(frw.WitnessEngine.groth16_prove_seeded_dev)
    for method in ("rerandomize_seeded_dev", "rerandomize_wire_seeded_dev"):
        assert callable(getattr(frw.Groth16Verifier, method))
    # what the header must say about what stays the caller's
    section = header[header.index("drawing the factors on the device (frw_drbg.h"):header.index("#define FRW_DRAW_BLINDING")]
    for phrase in ("SECRET", "NEVER recur", "restart", "same seed, counter and tag", "NOT constant-time", "does NOT advance the counter"):
        assert phrase in section, phrase


@pytest.mark.parametrize("counter", [0, 1 << 32, (1 << 64) - 1])
@pytest.mark.parametrize("tag", [0, 1, 2, 255])
def test_fr_draw_against_hashlib(counter, tag):
    lib = frw.load_library()
    seed = _seed()
    for count in (0, 1, 2, 65):
        buf = np.full((count + 2) * 4, GUARD, dtype=np.uint64)                  # guard words behind
        assert lib.frw_fr_draw(_ptr(seed), C.c_uint64(counter), tag, count, _ptr(buf)) == OK
        assert (buf[:4 * count].reshape(count, 4) == D.draw(D.SEED, counter, tag, count)).all(), count
        assert (buf[4 * count:] == GUARD).all(), count                           # count x 32 bytes and no more
        assert (frw.fr_draw(D.SEED, counter, tag, count) == D.draw(D.SEED, counter, tag, count)).all()
    assert bytes(seed) == D.SEED


def test_fr_draw_tags_and_seeds_are_separate():
    a, b = frw.fr_draw(D.SEED, 5, D.BLINDING, 16), frw.fr_draw(D.SEED, 5, D.RERANDOMIZE, 16)
    assert not set(map(bytes, a)) & set(map(bytes, b))
    other = bytes(31) + b"\x01"
    assert (frw.fr_draw(other, 5, 1, 4) == D.draw(other, 5, 1, 4)).all() and not (frw.fr_draw(other, 5, 1, 4) == a[:4]).all()
    with pytest.raises(frw.FrwError):
        frw.fr_draw(b"short", 0, 1, 1)
    with pytest.raises(frw.FrwError):
        frw.fr_draw(D.SEED, 0, 256, 1)


def test_refusals_of_the_host_function():
    lib = frw.load_library()
    seed, out = _seed(), np.full(8, GUARD, dtype=np.uint64)
    assert lib.frw_fr_draw(None, C.c_uint64(0), 1, 1, _ptr(out)) == INVALID
    assert lib.frw_fr_draw(_ptr(seed), C.c_uint64(0), 1, 1, None) == INVALID
    for tag in (256, -1, 1 << 16):
        assert lib.frw_fr_draw(_ptr(seed), C.c_uint64(0), tag, 1, _ptr(out)) == INVALID, tag
    assert (out == GUARD).all()
    # count = 0: a no-op that returns before anything else is looked at
    assert lib.frw_fr_draw(None, C.c_uint64(0), 999, 0, None) == OK


def test_refusals_of_the_device_calls():
    """the refusals that need no device: null pointers, a bad tag, and count / batch = 0 before anything else is looked at; with good
    arguments a machine without a device says FRW_E_NO_DEVICE (no host fallback)"""
    lib = frw.load_library()
    buf = np.zeros(64, dtype=np.uint64)
    p = _ptr(buf)
    good = dict(device=0, seed=p, counter=p, tag=1, count=1, out=p, stream=None)
    call = lambda **kw: lib.frw_fr_draw_dev(*[dict(good, **kw)[k] for k in ("device", "seed", "counter", "tag", "count", "out", "stream")])
    for null in ("seed", "counter", "out"):
        assert call(**{null: None}) == INVALID, null
    for tag in (256, -1):
        assert call(tag=tag) == INVALID, tag
    assert call(count=0, seed=None, counter=None, out=None, tag=999, device=-7) == OK
    if lib.frw_device_count() <= 0:
        assert call() == NO_DEVICE
    assert call(device=-1) == NO_DEVICE and call(device=1 << 20) == NO_DEVICE
    assert (buf == 0).all()
    # the composed calls: batch = 0 first; then the pointers of the draw; then the wrapped call's refusals (a null key here)
    assert lib.frw_groth16_prove_seeded_dev(None, None, 0, None, None, None, None, None, None, None, None, 0, None) == OK
    assert lib.frw_groth16_rerandomize_seeded_dev(None, 0, None, None, None, None, 99, None, None, None, 0, None) == OK
    assert lib.frw_groth16_rerandomize_wire_seeded_dev(None, 0, None, 9, None, None, None, 99, None, None, None, 0, None) == OK
    for seed, counter, rs in ((None, p, p), (p, None, p), (p, p, None), (p, p, p)):
        assert lib.frw_groth16_prove_seeded_dev(None, None, 1, p, p, seed, counter, rs, p, None, p, 1 << 20, None) == INVALID
        assert lib.frw_groth16_rerandomize_seeded_dev(None, 1, p, seed, counter, rs, 0, p, p, p, 1 << 20, None) == INVALID
        assert lib.frw_groth16_rerandomize_wire_seeded_dev(None, 1, p, 0, seed, counter, rs, 0, p, p, p, 1 << 20, None) == INVALID
    assert (buf == 0).all()
