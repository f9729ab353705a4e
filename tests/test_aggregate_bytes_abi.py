"""The aggregate from bytes (frw_aggregate_screen_workspace_bytes, frw_aggregate_falcon_verify_from_bytes(_dev),
frw_aggregate_statement_from_bytes(_dev), frw_aggregate_prove_workspace_bytes, frw_aggregate_prove_from_bytes(_dev)) where no GPU is
needed: the symbols exist in the library, the header, the ctypes table and the Rust declarations; every argument the header says is
refused before a handle is looked into is refused with FRW_E_INVALID_ARG; the routing function (falcon-r1cs_amd/csrc/frw_layout.h
aggregate_route, compiled for the host through the test-only shim) gives Python's prefix sums for every statement of random lists; both
workspace layouts have aligned, disjoint pieces and grow with the counts; and a stand-alone program carves real memory by them, and
stages mixed-length inputs (frw_stage.h StagedAggregate), under AddressSanitizer and UndefinedBehaviorSanitizer.

The header names eight functions: two size functions, three device forms and three host forms.

"Before a handle is looked into": the context and the key below are zero bytes; the constraint system is 4,096 zero bytes, which reads
as a handle that is not an aggregate -- itself one of the refusals."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess

import pytest

import falcon_r1cs_amd as frw

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("frw_aggregate_screen_workspace_bytes", "frw_aggregate_falcon_verify_from_bytes_dev", "frw_aggregate_statement_from_bytes_dev",
       "frw_aggregate_prove_workspace_bytes", "frw_aggregate_prove_from_bytes_dev", "frw_aggregate_falcon_verify_from_bytes",
       "frw_aggregate_statement_from_bytes", "frw_aggregate_prove_from_bytes")
INVALID = -1
PK_LEN, SIG_LEN = {9: 897, 10: 1793}, {9: 666, 10: 1280}


def test_the_new_symbols_are_exported_and_declared():
    lib = C.CDLL(frw.lib_path())
    header = open(os.path.join(ROOT, "include", "frw.h")).read()
    rust = open(os.path.join(ROOT, "rust", "frw-sys", "src", "lib.rs")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in frw._lib.PROTOTYPES, name
        assert "pub fn %s(" % name in rust, name
    for method in ("aggregate_falcon_verify_from_bytes", "aggregate_falcon_verify_from_bytes_dev", "aggregate_statement_from_bytes",
                   "aggregate_statement_from_bytes_dev", "aggregate_prove_from_bytes", "aggregate_prove_from_bytes_dev",
                   "aggregate_screen_workspace_bytes", "aggregate_prove_workspace_bytes"):
        assert callable(getattr(frw.WitnessEngine, method))
    assert callable(frw.Groth16Verifier.verify_aggregate_wire_dev)
    # the header says what the call waits for, what it cannot check, and which way in is the checked one
    assert "THE ONE HOST WAIT" in header and "What the call CANNOT check" in header and "THE CHECKED WAY IN" in header


def test_the_header_still_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc
    flags = [cc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include")]
    subprocess.check_call(flags + [os.path.join(HERE, "c", "test_header_c99.c")])
    src = tmp_path / "agg.c"
    src.write_text('#include "frw.h"\n'
                   "size_t (*const a)(const frw_r1cs *) = frw_aggregate_screen_workspace_bytes;\n"
                   "size_t (*const b)(const frw_groth16_pk *, const frw_r1cs *) = frw_aggregate_prove_workspace_bytes;\n"
                   "int (*const c)(const frw_r1cs *, frw_ctx *, const uint8_t *, const uint8_t *, const uint8_t *, const uint64_t *, int, int32_t *,\n"
                   "               uint64_t *) = frw_aggregate_falcon_verify_from_bytes;\n"
                   "int main(void) { return a(0) != 0 || b(0, 0) != 0 || c == 0; }\n")
    subprocess.check_call(flags + [str(src)])


@pytest.fixture(scope="module")
def env():
    lib = frw.load_library()
    fake = [(C.c_uint8 * 4096)() for _ in range(3)]             # ctx, pk, r: zero bytes
    buf = (C.c_uint64 * 128)()                                  # stand-in for every other pointer: never dereferenced
    p = C.c_void_p((C.addressof(buf) + 255) & ~255)
    return lib, [C.cast(f, C.c_void_p) for f in fake], p, (fake, buf)


def _args(handles, p, null, **over):
    a = dict(ctx=handles[0], pk=handles[1], r=handles[2], pkb=p, second=p, msgs=p, off=p, rs=p, wire=p, proof=p, inst=p, non=p, st=p, uns=p,
             norm=p, ws=p)
    a.update(over)
    if null:
        a[null] = None
    return a


def _screen(lib, handles, p, null=None, rule=0, host=False, **over):
    a = _args(handles, p, null, **over)
    if host:
        return lib.frw_aggregate_falcon_verify_from_bytes(a["r"], a["ctx"], a["pkb"], a["second"], a["msgs"], a["off"], rule, a["st"], a["norm"])
    return lib.frw_aggregate_falcon_verify_from_bytes_dev(a["r"], a["ctx"], a["pkb"], a["second"], a["msgs"], a["off"], rule, a["st"], a["norm"],
                                                          a["ws"], 1 << 30, None)


def _statement(lib, handles, p, null=None, encoding=1, host=False, **over):
    a = _args(handles, p, null, **over)
    if host:
        return lib.frw_aggregate_statement_from_bytes(a["r"], a["ctx"], a["pkb"], a["second"], a["msgs"], a["off"], encoding, a["inst"], a["st"])
    return lib.frw_aggregate_statement_from_bytes_dev(a["r"], a["ctx"], a["pkb"], a["second"], a["msgs"], a["off"], encoding, a["inst"], a["st"],
                                                      a["ws"], 1 << 30, None)


def _prove(lib, handles, p, null=None, mode=0, host=False, **over):
    a = _args(handles, p, null, **over)
    if host:
        return lib.frw_aggregate_prove_from_bytes(a["ctx"], a["pk"], a["r"], a["pkb"], a["second"], a["msgs"], a["off"], a["rs"], mode, a["wire"],
                                                  a["proof"], a["inst"], a["non"], a["st"], a["uns"])
    return lib.frw_aggregate_prove_from_bytes_dev(a["ctx"], a["pk"], a["r"], a["pkb"], a["second"], a["msgs"], a["off"], a["rs"], mode, a["wire"],
                                                  a["proof"], a["inst"], a["non"], a["st"], a["uns"], a["ws"], 1 << 30, None)


@pytest.mark.parametrize("host", [False, True])
def test_null_pointers_and_a_null_handle_are_refused(env, host):
    lib, handles, p, _ = env
    for which in ("ctx", "r", "pkb", "second", "msgs", "off", "st") + (() if host else ("ws",)):
        assert _screen(lib, handles, p, null=which, host=host) == INVALID, which
    for which in ("ctx", "r", "pkb", "second", "msgs", "off", "inst", "st") + (() if host else ("ws",)):
        assert _statement(lib, handles, p, null=which, host=host) == INVALID, which
    for which in ("ctx", "pk", "r", "pkb", "second", "msgs", "off", "rs", "wire", "st") + (() if host else ("ws",)):
        assert _prove(lib, handles, p, null=which, host=host) == INVALID, which


@pytest.mark.parametrize("host", [False, True])
def test_a_bad_rule_encoding_or_wire_mode_is_refused(env, host):
    lib, handles, p, _ = env
    for rule in (2, -1, 17):
        assert _screen(lib, handles, p, rule=rule, host=host) == INVALID
    for encoding in (2, 3, -1):                                 # 2: FRW_ENC_COMPACT, there is no compact form of an instance vector
        assert _statement(lib, handles, p, encoding=encoding, host=host) == INVALID
    for mode in (2, -1):
        assert _prove(lib, handles, p, mode=mode, host=host) == INVALID


@pytest.mark.parametrize("host", [False, True])
def test_a_handle_that_is_not_an_aggregate_is_refused(env, host):
    lib, handles, p, _ = env
    assert _screen(lib, handles, p, host=host) == INVALID
    assert _statement(lib, handles, p, host=host) == INVALID
    assert _prove(lib, handles, p, host=host) == INVALID


def test_a_misaligned_workspace_is_refused(env):
    lib, handles, p, _ = env
    for shift in (1, 4, 8):
        assert _screen(lib, handles, p, ws=C.c_void_p(p.value + shift)) == INVALID
        assert _statement(lib, handles, p, ws=C.c_void_p(p.value + shift)) == INVALID
    for shift in (1, 16, 128):
        assert _prove(lib, handles, p, ws=C.c_void_p(p.value + shift)) == INVALID


def test_the_size_functions_are_zero_for_a_null_or_foreign_handle(env):
    lib, handles, p, _ = env
    assert lib.frw_aggregate_screen_workspace_bytes(None) == 0
    assert lib.frw_aggregate_screen_workspace_bytes(handles[2]) == 0
    assert lib.frw_aggregate_prove_workspace_bytes(None, None) == 0
    assert lib.frw_aggregate_prove_workspace_bytes(handles[1], None) == 0
    assert lib.frw_aggregate_prove_workspace_bytes(None, handles[2]) == 0
    assert lib.frw_aggregate_prove_workspace_bytes(handles[1], handles[2]) == 0


# ---- the routing function and the layouts, through the shim ----------------------------------------------------------------------------
SRC = os.path.join(HERE, "cpp", "test_aggregate_bytes.cpp")
HDRS = [os.path.join(ROOT, "falcon-r1cs_amd", "csrc", h) for h in ("frw_layout.h", "frw_stage.h")]
INC = ["-I", os.path.join(HERE, "cpp", "hip_host"), "-I", os.path.join(ROOT, "falcon-r1cs_amd", "csrc")]


@pytest.fixture(scope="module")
def shim():
    out = os.path.join(HERE, "cpp", "build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libtest_aggregate_bytes.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror"] + INC + ["-o", so, SRC])
    lib = C.CDLL(so)
    for name in ("t_agg_pk_bytes", "t_agg_sig_bytes", "t_agg_screen", "t_agg_prove"):
        getattr(lib, name).restype = C.c_uint64
    lib.t_agg_route.restype = None
    return lib


def _routes(shim, logns):
    """[(pk_off, sig_off, nonce_off)] per statement from the header's function: item k of set g is the k-th statement of that set"""
    seen = {9: 0, 10: 0}
    out = []
    for s, l in enumerate(logns):
        r = (C.c_uint64 * 3)()
        shim.t_agg_route(l - 9, C.c_uint64(seen[l]), C.c_uint64(s), r)
        seen[l] += 1
        out.append(tuple(int(x) for x in r))
    return out


def test_every_statement_is_where_the_prefix_sums_say(shim):
    rng = random.Random(20261019)
    lists = [(9,), (10,), (9, 10, 9), (10, 9, 10)] + [tuple(rng.choice((9, 10)) for _ in range(rng.randint(1, 40))) for _ in range(200)]
    for logns in lists:
        pk_at = sig_at = 0
        want = []
        for s, l in enumerate(logns):
            want.append((pk_at, sig_at, 40 * s))
            pk_at += PK_LEN[l]
            sig_at += SIG_LEN[l]
        assert _routes(shim, logns) == want, logns
        c9, c10 = logns.count(9), logns.count(10)
        assert int(shim.t_agg_pk_bytes(C.c_uint64(c9), C.c_uint64(c10))) == pk_at, logns
        assert int(shim.t_agg_sig_bytes(C.c_uint64(c9), C.c_uint64(c10))) == sig_at, logns


W_OF, N_OF = {9: 153 * 512 + 50, 10: 153 * 1024 + 52}, {9: 512, 10: 1024}


def _screen_layout(shim, c9, c10):
    n = shim.t_agg_screen_pieces()
    out = (C.c_uint64 * (2 * n))()
    size = int(shim.t_agg_screen(C.c_uint64(c9), C.c_uint64(c10), out))
    return size, [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)]


def _prove_layout(shim, c9, c10, g16):
    n = shim.t_agg_prove_pieces()
    out = (C.c_uint64 * (2 * n + 4))()
    size = int(shim.t_agg_prove(C.c_uint64(c9), C.c_uint64(c10), C.c_uint64(g16), out))
    v = [int(x) for x in out]
    return size, [(v[2 * i], v[2 * i + 1]) for i in range(n + 1)], v[2 * n + 2], v[2 * n + 3]


def _in_order(pieces, size):
    ends = [off + ln for off, ln in pieces]
    return all(e <= nxt for e, nxt in zip(ends, [off for off, _ in pieces[1:]] + [size]))


COUNTS = [(1, 0), (0, 1), (2, 1), (1, 2), (4, 3), (290, 10), (513, 511), (0, 0)]


def test_the_screen_layout_has_aligned_disjoint_pieces_inside_its_size(shim):
    for c9, c10 in COUNTS:
        size, pieces = _screen_layout(shim, c9, c10)
        assert len(pieces) == 16 and size % 16 == 0
        assert all(off % 16 == 0 for off, _ in pieces) and _in_order(pieces, size), (c9, c10)
        per = lambda c, n: [2 * n * c] * 3 + [4 * c] * 3 + [8 * c]
        assert [ln for _, ln in pieces] == per(c9, 512) + per(c10, 1024) + [40 * (c9 + c10), 4]


def test_the_prove_layout_has_aligned_disjoint_pieces_inside_its_size(shim):
    for c9, c10 in COUNTS:
        g16 = 256 * 1001
        size, pieces, W, I = _prove_layout(shim, c9, c10, g16)
        assert len(pieces) == 30 and size % 256 == 0
        assert all(off % 16 == 0 for off, _ in pieces) and _in_order(pieces, size), (c9, c10)
        assert W == c9 * W_OF[9] + c10 * W_OF[10] and I == 1 + 2 * (512 * c9 + 1024 * c10)
        # the screen's pieces are the screen layout's own, at the head
        assert pieces[:16] == _screen_layout(shim, c9, c10)[1]
        # what the prover and the witness kernels take starts on 256-byte boundaries
        assert all(pieces[i][0] % 256 == 0 for i in (16, 19, 22, 29)) and pieces[29][1] == g16
        assert [ln for _, ln in pieces[16:29]] == [32 * W_OF[9] * c9, 32 * 1025 * c9, 4 * c9, 32 * W_OF[10] * c10, 32 * 2049 * c10, 4 * c10,
                                                   32 * W, 32 * I, 384, 384, 4, 4, 4 * (c9 + c10)]


def test_the_sizes_are_monotone_in_the_counts(shim):
    for other in (0, 1, 7):
        for which in (0, 1):
            counts = [(c, other) if which == 0 else (other, c) for c in (0, 1, 2, 3, 9, 255, 256, 257, 1030)]
            screen = [_screen_layout(shim, *c)[0] for c in counts]
            prove = [_prove_layout(shim, c[0], c[1], 4096)[0] for c in counts]
            assert screen == sorted(screen) and len(set(screen)) == len(screen)
            assert prove == sorted(prove) and len(set(prove)) == len(prove)
    sizes = [_prove_layout(shim, 2, 1, g)[0] for g in (256, 512, 4096, 1 << 20)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)


def test_layouts_and_staging_are_clean_under_the_sanitizers(tmp_path):
    """The stand-alone program of tests/cpp/test_aggregate_bytes.cpp (its own main, nothing of it is loaded into Python), built with
    -fsanitize=address,undefined: both layouts carved over allocations of exactly the reported size, and StagedAggregate filled from
    sources exactly as long as a caller's."""
    exe = str(tmp_path / "aggregate_bytes_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Werror"] + INC + ["-o", exe, SRC])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert res.returncode == 0, res.stdout
    assert res.stdout.strip().endswith("aggregate_bytes: clean"), res.stdout
    assert "20 aggregates staged" in res.stdout
