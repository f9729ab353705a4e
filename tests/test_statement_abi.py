"""The statement entry points' C ABI where no GPU is needed (frw_statement_dev, frw_statement, frw_statement_workspace_bytes,
frw_statement_from_bytes_dev, frw_statement_from_bytes, frw_aggregate_statement_dev): the symbols exist, every argument the header says
is refused is refused with FRW_E_INVALID_ARG before any device is touched, and the workspace of the bytes path is laid out as
tests/golden/statement_layout.json says (falcon-r1cs_amd/csrc/frw_layout.h compiled for the host through the test-only shim).

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
NEW = ("frw_statement_dev", "frw_statement", "frw_statement_workspace_bytes", "frw_statement_from_bytes_dev", "frw_statement_from_bytes",
       "frw_aggregate_statement_dev")
INVALID = -1
ENC_COMPACT = 2


def test_the_new_symbols_are_exported_and_declared():
    lib = C.CDLL(frw.lib_path())
    header = open(os.path.join(ROOT, "include", "frw.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in header, name
        assert name in frw._lib.PROTOTYPES, name
    # the header tells a downstream verifier what a refused statement looks like to it
    assert "instance[0] != 1" in header


@pytest.fixture(scope="module")
def env():
    lib = frw.load_library()
    fake_ctx = (C.c_uint8 * 256)()
    buf = (C.c_uint64 * 64)()                    # 16-byte aligned stand-in for every pointer: never dereferenced
    p = C.cast(buf, C.c_void_p)
    assert p.value % 16 == 0
    return lib, C.cast(fake_ctx, C.c_void_p), p


def _dev(lib, ctx, p, circuit=0, logn=9, batch=1, pk=True, hm=True, enc=1, inst=True, st=True):
    P = lambda on: p if on else None
    return lib.frw_statement_dev(ctx, circuit, logn, batch, P(pk), P(hm), enc, P(inst), P(st), None)


def _host(lib, ctx, p, circuit=0, logn=9, batch=1, pk=True, hm=True, enc=1, inst=True, st=True):
    P = lambda on: p if on else None
    return lib.frw_statement(ctx, circuit, logn, batch, P(pk), P(hm), enc, P(inst), P(st), 1)


def _bytes_dev(lib, ctx, p, circuit=0, logn=9, batch=1, enc=1, null=None, ws=None, ws_bytes=None):
    args = dict(pkb=p, non=p, msgs=p, off=p, inst=p, st=p, ws=p if ws is None else ws)
    if null:
        args[null] = None
    need = lib.frw_statement_workspace_bytes(logn, batch)
    return lib.frw_statement_from_bytes_dev(ctx, circuit, logn, batch, args["pkb"], args["non"], args["msgs"], args["off"], enc, args["inst"],
                                            args["st"], args["ws"], need if ws_bytes is None else ws_bytes, None)


def _bytes_host(lib, ctx, p, circuit=0, logn=9, batch=1, enc=1, null=None, off=None):
    args = dict(pkb=p, non=p, msgs=p, off=p if off is None else off, inst=p, st=p)
    if null:
        args[null] = None
    return lib.frw_statement_from_bytes(ctx, circuit, logn, batch, args["pkb"], args["non"], args["msgs"], args["off"], enc, args["inst"],
                                        args["st"], 1)


@pytest.mark.parametrize("call", [_dev, _host, _bytes_dev, _bytes_host])
def test_bad_encoding_circuit_and_logn_are_refused(env, call):
    lib, ctx, p = env
    for enc in (ENC_COMPACT, 3, -1):
        assert call(lib, ctx, p, enc=enc) == INVALID
    for circuit in (3, -1, 17):
        assert call(lib, ctx, p, circuit=circuit) == INVALID
    for logn in (8, 11, 0):
        assert call(lib, ctx, p, logn=logn) == INVALID
    assert call(lib, None, p) == INVALID                    # no context
    for batch in (0, 1):                                    # the arguments are looked at whatever the batch
        assert call(lib, ctx, p, batch=batch, enc=ENC_COMPACT) == INVALID


def test_null_pointers_are_refused(env):
    lib, ctx, p = env
    for call in (_dev, _host):
        for which in ("pk", "hm", "inst", "st"):
            assert call(lib, ctx, p, **{which: False}) == INVALID
    for which in ("pkb", "non", "msgs", "off", "inst", "st", "ws"):
        assert _bytes_dev(lib, ctx, p, null=which) == INVALID
    for which in ("pkb", "non", "off", "inst", "st"):
        assert _bytes_host(lib, ctx, p, null=which) == INVALID


def test_small_or_misaligned_workspace_is_refused(env):
    lib, ctx, p = env
    for logn in (9, 10):
        need = lib.frw_statement_workspace_bytes(logn, 3)
        assert need > 0
        assert _bytes_dev(lib, ctx, p, logn=logn, batch=3, ws_bytes=need - 1) == INVALID
        assert _bytes_dev(lib, ctx, p, logn=logn, batch=3, ws_bytes=0) == INVALID
        for shift in (1, 4, 8):
            assert _bytes_dev(lib, ctx, p, logn=logn, batch=3, ws=C.c_void_p(p.value + shift), ws_bytes=need + 16) == INVALID


def test_decreasing_message_offsets_are_refused(env):
    lib, ctx, p = env
    off = (C.c_uint64 * 3)(0, 8, 4)
    assert _bytes_host(lib, ctx, p, batch=2, off=C.cast(off, C.c_void_p)) == INVALID


def test_the_aggregate_form_refuses_what_is_no_aggregate(env):
    lib, ctx, p = env
    # no handle (an aggregate handle needs a device to exist), no context
    assert lib.frw_aggregate_statement_dev(None, ctx, p, p, p, p, 1, p, p, None) == INVALID
    assert lib.frw_aggregate_statement_dev(None, None, p, p, p, p, 1, p, p, None) == INVALID
    assert lib.frw_aggregate_statement_dev(None, ctx, p, p, p, p, ENC_COMPACT, p, p, None) == INVALID


# ---- the workspace layout ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim():
    out = os.path.join(HERE, "cpp", "build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libtest_statement_layout.so")
    src = os.path.join(HERE, "cpp", "test_statement_layout.cpp")
    hdr = os.path.join(ROOT, "falcon-r1cs_amd", "csrc", "frw_layout.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in (src, hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(HERE, "cpp", "hip_host"),
                               "-I", os.path.join(ROOT, "falcon-r1cs_amd", "csrc"), "-o", so, src])
    lib = C.CDLL(so)
    lib.t_statement.restype = C.c_uint64
    return lib


def test_workspace_layout_matches_the_golden_file(shim):
    with open(os.path.join(HERE, "golden", "statement_layout.json")) as f:
        cases = json.load(f)["cases"]
    assert sorted({c["logn"] for c in cases}) == [9, 10] and len(cases) >= 16
    lib = frw.load_library()
    for c in cases:
        out = (C.c_uint64 * 3)()
        size = shim.t_statement(c["logn"], C.c_uint64(c["batch"]), out)
        assert [int(x) for x in out] == [c["pk"], c["hm"], c["decode_status"]], c
        assert size == c["bytes"] == lib.frw_statement_workspace_bytes(c["logn"], c["batch"]), c
        # the pieces are 16-byte aligned, disjoint and inside the workspace
        n = 1 << c["logn"]
        assert all(int(x) % 16 == 0 for x in out) and size % 16 == 0
        assert c["pk"] + 2 * n * c["batch"] <= c["hm"] and c["hm"] + 2 * n * c["batch"] <= c["decode_status"]
        assert c["decode_status"] + 4 * c["batch"] <= size
    for logn in (8, 11):
        assert lib.frw_statement_workspace_bytes(logn, 4) == 0
