"""The prover from bytes (frw_pok_prove_workspace_bytes, frw_pok_prove_from_bytes_dev, frw_pok_prove_from_bytes) where no GPU is needed:
the symbols exist in the library, the header, the ctypes table and the Rust declarations; every argument the header says is refused
before a handle is looked at is refused with FRW_E_INVALID_ARG; the workspace layout (falcon-r1cs_amd/csrc/frw_layout.h
pok_prove_layout, compiled for the host through the test-only shim) has aligned, disjoint pieces and grows with the batch and with the
proofs in flight; and a stand-alone program carves real memory by it under AddressSanitizer and UndefinedBehaviorSanitizer.

"Before a handle is looked at": the context, the key and the constraint system below are 256 zero bytes each.  The checks exercised
here never look inside them; a call that got past them would read a handle's fields, which none of these does."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import falcon_r1cs_amd as frw

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ("frw_pok_prove_workspace_bytes", "frw_pok_prove_from_bytes_dev", "frw_pok_prove_from_bytes")
INVALID = -1
SIG_LEN = 666


def test_the_new_symbols_are_exported_and_declared():
    lib = C.CDLL(frw.lib_path())
    header = open(os.path.join(ROOT, "include", "frw.h")).read()
    rust = open(os.path.join(ROOT, "rust", "frw-sys", "src", "lib.rs")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in frw._lib.PROTOTYPES, name
        assert "pub fn %s(" % name in rust, name
    for method in ("pok_prove_workspace_bytes", "pok_prove_from_bytes_dev", "pok_prove_from_bytes"):
        assert callable(getattr(frw.WitnessEngine, method))
    # the header says that the call waits on the host once and is not capture-safe
    assert "THE ONE HOST WAIT" in header and "NOT stream-capture safe" in header


def test_the_header_still_compiles_as_c99(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "c", "test_header_c99.c")])
    src = tmp_path / "pok.c"
    src.write_text('#include "frw.h"\n'
                   "size_t (*const a)(const frw_groth16_pk *, const frw_r1cs *, int, int, size_t, size_t) = frw_pok_prove_workspace_bytes;\n"
                   "int main(void) { return a(0, 0, 0, 9, 1, 1) != 0; }\n")
    subprocess.check_call([cc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


@pytest.fixture(scope="module")
def env():
    lib = frw.load_library()
    fake = [(C.c_uint8 * 256)() for _ in range(3)]              # ctx, pk, r: never looked into by the checks below
    buf = (C.c_uint64 * 128)()                                  # stand-in for every other pointer: never dereferenced
    p = C.c_void_p((C.addressof(buf) + 255) & ~255)
    assert p.value % 256 == 0
    return lib, [C.cast(f, C.c_void_p) for f in fake], p, (fake, buf)


def _dev(lib, handles, p, circuit=0, logn=9, batch=1, mode=0, null=None, ws=None, ws_bytes=1 << 30, sig_len=SIG_LEN):
    a = dict(ctx=handles[0], pk=handles[1], r=handles[2], pkb=p, sgb=p, msgs=p, off=p, rs=p, wire=p, proofs=p, inst=p, st=p, uns=p,
             ws=p if ws is None else ws)
    if null:
        a[null] = None
    return lib.frw_pok_prove_from_bytes_dev(a["ctx"], a["pk"], a["r"], circuit, logn, batch, a["pkb"], a["sgb"], sig_len, a["msgs"], a["off"],
                                            a["rs"], mode, a["wire"], a["proofs"], a["inst"], a["st"], a["uns"], a["ws"], ws_bytes, None)


def _host(lib, handles, p, circuit=0, logn=9, batch=1, mode=0, null=None, off=None, sig_len=SIG_LEN):
    a = dict(ctx=handles[0], pk=handles[1], r=handles[2], pkb=p, sgb=p, msgs=p, off=p if off is None else off, rs=p, wire=p, proofs=p,
             inst=p, st=p, uns=p)
    if null:
        a[null] = None
    return lib.frw_pok_prove_from_bytes(a["ctx"], a["pk"], a["r"], circuit, logn, batch, a["pkb"], a["sgb"], sig_len, a["msgs"], a["off"],
                                        a["rs"], mode, a["wire"], a["proofs"], a["inst"], a["st"], a["uns"], 1)


@pytest.mark.parametrize("call", [_dev, _host])
def test_bad_logn_circuit_wire_mode_and_context_are_refused(env, call):
    lib, handles, p, _ = env
    for batch in (0, 1):                                        # these are looked at whatever the batch
        for logn in (8, 11, 0, -1):
            assert call(lib, handles, p, logn=logn, batch=batch) == INVALID
        for circuit in (3, -1, 17):
            assert call(lib, handles, p, circuit=circuit, batch=batch) == INVALID
        for mode in (2, -1):
            assert call(lib, handles, p, mode=mode, batch=batch) == INVALID
        for sig_len in (0, 1, 40, 41):
            assert call(lib, handles, p, sig_len=sig_len, batch=batch) == INVALID
        assert call(lib, handles, p, null="ctx", batch=batch) == INVALID


def test_null_pointers_are_refused(env):
    lib, handles, p, _ = env
    for batch in (0, 1):
        for which in ("pk", "r", "pkb", "sgb", "msgs", "off", "rs", "wire", "st", "ws"):
            assert _dev(lib, handles, p, null=which, batch=batch) == INVALID, which
        for which in ("pk", "r", "pkb", "sgb", "msgs", "off", "rs", "wire", "st"):
            assert _host(lib, handles, p, null=which, batch=batch) == INVALID, which


def test_batch_zero_is_a_no_op_also_without_the_optional_outputs(env):
    lib, handles, p, _ = env
    for call in (_dev, _host):
        assert call(lib, handles, p, batch=0) == 0
        for which in ("proofs", "inst", "uns"):
            assert call(lib, handles, p, batch=0, null=which) == 0


def test_a_misaligned_workspace_is_refused(env):
    lib, handles, p, _ = env
    for shift in (1, 8, 16, 128):
        for batch in (0, 1):
            assert _dev(lib, handles, p, ws=C.c_void_p(p.value + shift), batch=batch) == INVALID


def test_decreasing_message_offsets_are_refused(env):
    lib, handles, p, _ = env
    off = (C.c_uint64 * 3)(0, 8, 4)
    assert _host(lib, handles, p, batch=2, off=C.cast(off, C.c_void_p)) == INVALID


def test_workspace_bytes_is_zero_for_bad_arguments(env):
    lib, handles, p, _ = env
    f = lib.frw_pok_prove_workspace_bytes
    assert f(None, handles[2], 0, 9, 4, 1) == 0 and f(handles[1], None, 0, 9, 4, 1) == 0
    for logn in (8, 11):
        assert f(handles[1], handles[2], 0, logn, 4, 1) == 0
    for circuit in (3, -1):
        assert f(handles[1], handles[2], circuit, 9, 4, 1) == 0
    assert f(handles[1], handles[2], 0, 9, 4, 0) == 0           # nothing in flight


# ---- the workspace layout ---------------------------------------------------------------------------------------------------------------
SRC = os.path.join(HERE, "cpp", "test_pok_prove_layout.cpp")
HDR = os.path.join(ROOT, "falcon-r1cs_amd", "csrc", "frw_layout.h")
INC = ["-I", os.path.join(HERE, "cpp", "hip_host"), "-I", os.path.join(ROOT, "falcon-r1cs_amd", "csrc")]


@pytest.fixture(scope="module")
def shim():
    out = os.path.join(HERE, "cpp", "build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libtest_pok_prove_layout.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in (SRC, HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror"] + INC + ["-o", so, SRC])
    lib = C.CDLL(so)
    lib.t_pok_prove.restype = C.c_uint64
    return lib


def _layout(shim, logn, batch, k, W, g16):
    n = shim.t_pok_prove_pieces()
    out = (C.c_uint64 * (2 * n + 4))()
    size = shim.t_pok_prove(logn, C.c_uint64(batch), C.c_uint64(k), C.c_uint64(W), C.c_uint64(g16), out)
    v = [int(x) for x in out]
    pieces = [(v[2 * i], v[2 * i + 1]) for i in range(n + 1)]   # the Groth16 workspace last
    return size, pieces, v[2 * n + 2], v[2 * n + 3]


W_OF = {9: 153 * 512 + 50, 10: 153 * 1024 + 52, "schoolbook9": 512 * 512 + 99 * 512 + 50}


@pytest.mark.parametrize("logn,W", [(9, W_OF[9]), (10, W_OF[10]), (9, W_OF["schoolbook9"])])
def test_pieces_are_aligned_disjoint_and_inside_the_workspace(shim, logn, W):
    n = 1 << logn
    for batch in (0, 1, 3, 9, 255, 256, 257, 1030, 70000):
        for k in (1, 2, 9, 64):
            g16 = 256 * (1000 * k + 1)
            size, pieces, fixed, per = _layout(shim, logn, batch, k, W, g16)
            assert len(pieces) == 21
            assert all(off % 16 == 0 for off, _ in pieces) and size % 16 == 0
            ends = [off + ln for off, ln in pieces]
            assert all(e <= nxt for e, nxt in zip(ends, [off for off, _ in pieces[1:]] + [size])), (batch, k)     # in order, no overlap
            # the witness and the prover's workspace start on 256-byte boundaries (the prover asks for that)
            assert pieces[10][0] % 256 == 0 and pieces[20][0] % 256 == 0 and pieces[20][1] == g16
            # the fixed part holds what is proportional to the batch, the rest what is proportional to the proofs in flight
            assert pieces[9][0] + pieces[9][1] <= fixed <= pieces[10][0]
            assert fixed >= batch * (3 * 2 * n + 40 + 4 + 4 + 4 + 64)
            assert per >= k * (32 * W + 32 * (2 * n + 1) + 3 * 2 * n + 384 + 384 + 12)
            assert size >= fixed + per + g16
            # the lengths are the arrays' own
            assert [ln for _, ln in pieces[:10]] == [2 * n * batch] * 3 + [40 * batch, 4 * batch, 4 * batch, 4 * batch, 4 * ((batch + 255) // 256), 4, 64 * batch]
            assert [ln for _, ln in pieces[10:20]] == [32 * W * k, 32 * (2 * n + 1) * k] + [2 * n * k] * 3 + [384 * k, 384 * k, 4 * k, 4 * k, 4 * k]


def test_the_size_is_monotone_in_the_batch_and_in_the_proofs_in_flight(shim):
    for logn in (9, 10):
        W = W_OF[logn]
        g16 = lambda k: 256 * (1000 * k + 1)                    # (the prover's own workspace grows with k, or stays: a key of bare handles)
        for k in (1, 2, 5):
            sizes = [_layout(shim, logn, b, k, W, g16(k))[0] for b in (0, 1, 2, 3, 9, 255, 256, 257, 1030, 4096)]
            assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
        for batch in (1, 9, 1030):
            sizes = [_layout(shim, logn, batch, k, W, g16(k))[0] for k in range(1, 12)]
            assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
            flat = [_layout(shim, logn, batch, k, W, 4096)[0] for k in range(1, 12)]
            assert flat == sorted(flat) and len(set(flat)) == len(flat)
        # the fixed part does not depend on the proofs in flight
        assert len({_layout(shim, logn, 1030, k, W, g16(k))[2] for k in (1, 2, 64)}) == 1


def test_the_layout_carves_real_memory_cleanly_under_the_sanitizers(tmp_path):
    """The stand-alone program of tests/cpp/test_pok_prove_layout.cpp (its own main, nothing of it is loaded into Python), built with
    -fsanitize=address,undefined: every piece written to its last byte inside an allocation of exactly the reported size."""
    exe = str(tmp_path / "pok_prove_layout_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Werror"] + INC + ["-o", exe, SRC])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert res.returncode == 0, res.stdout
    assert res.stdout.strip().endswith("pok_prove_layout: clean"), res.stdout
