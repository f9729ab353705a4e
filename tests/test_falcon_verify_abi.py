"""The Falcon verification entry points' C ABI where no GPU is needed (frw_falcon_verify_dev, frw_falcon_verify,
frw_falcon_verify_workspace_bytes, frw_falcon_verify_from_bytes_dev, frw_falcon_verify_from_bytes): the symbols exist, every argument the
header says is refused is refused with FRW_E_INVALID_ARG before any device is touched, and the workspace of the bytes path is laid out
as tests/golden/falcon_verify_layout.json says (falcon-r1cs_amd/csrc/frw_layout.h compiled for the host through the test-only shim).

"Before any device is touched": the calls below get a context that is 256 zero bytes.  The argument checks never look inside it; a call
that got past them would select a device and fail with FRW_E_HIP / FRW_E_NO_DEVICE on the CPU box (or run on a GPU box), never return
FRW_E_INVALID_ARG."""
import ctypes as C
import json
import os
import subprocess

import pytest

import falcon_r1cs_amd as frw

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("frw_falcon_verify_dev", "frw_falcon_verify", "frw_falcon_verify_workspace_bytes", "frw_falcon_verify_from_bytes_dev",
       "frw_falcon_verify_from_bytes")
INVALID = -1
SIG_LEN = 666


def test_the_new_symbols_are_exported_and_declared():
    lib = C.CDLL(frw.lib_path())
    header = open(os.path.join(ROOT, "include", "frw.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in header, name
        assert name in frw._lib.PROTOTYPES, name
    assert "#define FRW_RULE_CIRCUIT 0" in header and "#define FRW_RULE_SPEC    1" in header
    assert (frw.RULE_CIRCUIT, frw.RULE_SPEC) == (0, 1)
    # the header says where the two rules differ
    assert "differ in exactly two cases" in header and "6144^2 > beta^2 at Falcon-512" in header


@pytest.fixture(scope="module")
def env():
    lib = frw.load_library()
    fake_ctx = (C.c_uint8 * 256)()
    buf = (C.c_uint64 * 64)()                    # 16-byte aligned stand-in for every pointer: never dereferenced
    p = C.cast(buf, C.c_void_p)
    assert p.value % 16 == 0
    return lib, C.cast(fake_ctx, C.c_void_p), p


def _dev(lib, ctx, p, logn=9, batch=1, rule=0, null=None):
    a = dict(sig=p, pk=p, hm=p, st=p, norm=p)
    if null:
        a[null] = None
    return lib.frw_falcon_verify_dev(ctx, logn, batch, a["sig"], a["pk"], a["hm"], rule, a["st"], a["norm"], None)


def _host(lib, ctx, p, logn=9, batch=1, rule=0, null=None):
    a = dict(sig=p, pk=p, hm=p, st=p, norm=p)
    if null:
        a[null] = None
    return lib.frw_falcon_verify(ctx, logn, batch, a["sig"], a["pk"], a["hm"], rule, a["st"], a["norm"], 1)


def _bytes_dev(lib, ctx, p, logn=9, batch=1, rule=0, null=None, ws=None, ws_bytes=None, sig_len=SIG_LEN):
    a = dict(pkb=p, sgb=p, msgs=p, off=p, st=p, norm=p, ws=p if ws is None else ws)
    if null:
        a[null] = None
    need = lib.frw_falcon_verify_workspace_bytes(logn, batch)
    return lib.frw_falcon_verify_from_bytes_dev(ctx, logn, batch, a["pkb"], a["sgb"], sig_len, a["msgs"], a["off"], rule, a["st"], a["norm"],
                                                a["ws"], need if ws_bytes is None else ws_bytes, None)


def _bytes_host(lib, ctx, p, logn=9, batch=1, rule=0, null=None, off=None, sig_len=SIG_LEN):
    a = dict(pkb=p, sgb=p, msgs=p, off=p if off is None else off, st=p, norm=p)
    if null:
        a[null] = None
    return lib.frw_falcon_verify_from_bytes(ctx, logn, batch, a["pkb"], a["sgb"], sig_len, a["msgs"], a["off"], rule, a["st"], a["norm"], 1)


@pytest.mark.parametrize("call", [_dev, _host, _bytes_dev, _bytes_host])
def test_bad_logn_rule_and_context_are_refused(env, call):
    lib, ctx, p = env
    for logn in (8, 11, 0, -1):
        assert call(lib, ctx, p, logn=logn) == INVALID
    for rule in (2, -1, 17):
        assert call(lib, ctx, p, rule=rule) == INVALID
    assert call(lib, None, p) == INVALID                    # no context
    for batch in (0, 1):                                    # the arguments are looked at whatever the batch
        assert call(lib, ctx, p, batch=batch, rule=2) == INVALID
        assert call(lib, ctx, p, batch=batch, logn=11) == INVALID


def test_null_pointers_are_refused(env):
    lib, ctx, p = env
    for call in (_dev, _host):
        for which in ("sig", "pk", "hm", "st"):
            assert call(lib, ctx, p, null=which) == INVALID
    for which in ("pkb", "sgb", "msgs", "off", "st", "ws"):
        assert _bytes_dev(lib, ctx, p, null=which) == INVALID
    for which in ("pkb", "sgb", "msgs", "off", "st"):
        assert _bytes_host(lib, ctx, p, null=which) == INVALID


def test_a_null_norm_is_no_refusal(env):
    """d_norm may be NULL: with batch = 0 such a call is the no-op the header promises (FRW_OK, no device touched), not a refusal"""
    lib, ctx, p = env
    for call in (_dev, _host, _bytes_dev, _bytes_host):
        assert call(lib, ctx, p, batch=0, null="norm") == 0
        assert call(lib, ctx, p, batch=0) == 0


def test_small_or_misaligned_workspace_is_refused(env):
    lib, ctx, p = env
    for logn in (9, 10):
        need = lib.frw_falcon_verify_workspace_bytes(logn, 3)
        assert need > 0
        assert _bytes_dev(lib, ctx, p, logn=logn, batch=3, ws_bytes=need - 1) == INVALID
        assert _bytes_dev(lib, ctx, p, logn=logn, batch=3, ws_bytes=0) == INVALID
        for shift in (1, 4, 8):
            assert _bytes_dev(lib, ctx, p, logn=logn, batch=3, ws=C.c_void_p(p.value + shift), ws_bytes=need + 16) == INVALID


def test_a_signature_length_without_a_body_is_refused(env):
    lib, ctx, p = env
    for sig_len in (0, 1, 40, 41):
        assert _bytes_dev(lib, ctx, p, sig_len=sig_len) == INVALID
        assert _bytes_host(lib, ctx, p, sig_len=sig_len) == INVALID


def test_decreasing_message_offsets_are_refused(env):
    lib, ctx, p = env
    off = (C.c_uint64 * 3)(0, 8, 4)
    assert _bytes_host(lib, ctx, p, batch=2, off=C.cast(off, C.c_void_p)) == INVALID


# ---- the workspace layout ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    out = os.path.join(HERE, "cpp", "build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libtest_falcon_verify_layout.so")
    src = os.path.join(HERE, "cpp", "test_falcon_verify_layout.cpp")
    hdr = os.path.join(ROOT, "falcon-r1cs_amd", "csrc", "frw_layout.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in (src, hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(HERE, "cpp", "hip_host"),
                               "-I", os.path.join(ROOT, "falcon-r1cs_amd", "csrc"), "-o", so, src])
    lib = C.CDLL(so)
    lib.t_falcon_verify.restype = C.c_uint64
    return lib


def test_workspace_layout_matches_the_golden_file(shim):
    with open(os.path.join(HERE, "golden", "falcon_verify_layout.json")) as f:
        cases = json.load(f)["cases"]
    assert sorted({c["logn"] for c in cases}) == [9, 10] and len(cases) >= 16
    lib = frw.load_library()
    names = ("sig", "pk", "hm", "nonce", "sig_status", "pk_status")
    for c in cases:
        out = (C.c_uint64 * 6)()
        size = shim.t_falcon_verify(c["logn"], C.c_uint64(c["batch"]), out)
        assert [int(x) for x in out] == [c[k] for k in names], c
        assert size == c["bytes"] == lib.frw_falcon_verify_workspace_bytes(c["logn"], c["batch"]), c
        # the pieces are 16-byte aligned, disjoint, in this order and inside the workspace
        n, b = 1 << c["logn"], c["batch"]
        sizes = (2 * n * b, 2 * n * b, 2 * n * b, 40 * b, 4 * b, 4 * b)
        ends = [c[k] + s for k, s in zip(names, sizes)]
        assert all(int(x) % 16 == 0 for x in out) and size % 16 == 0
        assert all(e <= nxt for e, nxt in zip(ends, [c[k] for k in names[1:]] + [size])), c
    for logn in (8, 11):
        assert lib.frw_falcon_verify_workspace_bytes(logn, 4) == 0
