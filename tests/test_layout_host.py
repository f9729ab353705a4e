"""The workspace layouts of falcon-r1cs_amd/csrc/frw_layout.h, compiled for the host through the test-only shim (tests/cpp/hip_host):
every offset and size of the four MSM layouts against tests/golden/workspace_layouts.json (written from the carve functions of the
commit the golden file names, before the layouts moved into the header), the invariants the kernels rely on (arrays inside the workspace,
disjoint but for the documented borrowings, aligned for their widest access), and the prover's and the verification chains' compositions
against closed forms."""
import ctypes as C
import itertools
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ABSENT = (1 << 64) - 1
BW = {1: 60, 2: 116}                 # words of a bucket: G1, G2
B16, B8 = 32768, 128                 # buckets of a dense row, of a narrow window
NS = [1, 5, 63, 300, 1 << 18, (1 << 18) + 1]

DENSE = ["counts", "offsets", "order", "item_first", "item_count", "ones_count", "items", "buckets", "partial", "partial_items", "entries", "ones_list",
         "digits", "end", "window_sums", "bytes", "max_items", "ent_stride", "ones_stride"]
WIDE = ["partial_plain", "s1", "s0", "window_sums", "row_start", "bin_start", "row_count", "bin_count", "slice_hist", "coarse", "entries", "digits", "end", "bytes"]
NARROW = ["entry_base", "slice_hist", "counts", "offsets", "item_first", "items", "item_count", "ones_count", "ones_list", "entries", "partial_items",
          "partial_ones", "folded_ones", "bucket_sums", "window_sums", "end", "used", "bytes", "target", "max_items", "ones_stride", "sort_n"]
POINTS = ["A", "B1", "L", "H", "SA", "RB1", "B2", "rs", "split"]


def a16(x):
    return (x + 15) & ~15


def a256(x):
    return (x + 255) & ~255


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(HERE, "cpp", "build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libtest_layout.so")
    src = os.path.join(HERE, "cpp", "test_layout.cpp")
    hdr = os.path.join(ROOT, "falcon-r1cs_amd", "csrc", "frw_layout.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in (src, hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(HERE, "cpp", "hip_host"),
                               "-I", os.path.join(ROOT, "falcon-r1cs_amd", "csrc"), "-o", so, src])
    lib = C.CDLL(so)
    for name in ("t_points", "t_points_bytes", "t_groth16", "t_groth16_bare", "t_verify", "t_in_flight"):
        getattr(lib, name).restype = C.c_uint64
    return lib


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "workspace_layouts.json")) as f:
        return json.load(f)


def u64(*v):
    return [C.c_uint64(x) for x in v]


def call(fn, names, *args):
    out = (C.c_uint64 * 40)()
    fn(*args, out)
    return {k: int(out[i]) for i, k in enumerate(names) if int(out[i]) != ABSENT}


def dense(lib, group, rows, n, bare):
    return call(lib.t_dense, DENSE, group, C.c_uint64(rows), C.c_uint32(n), int(bare))


def wide(lib, group, n):
    out = (C.c_uint64 * 40)()
    lib.t_wide(group, C.c_uint32(n), out)
    rows = {k: int(out[i]) for i, k in enumerate(DENSE) if int(out[i]) != ABSENT}
    own = {k: int(out[len(DENSE) + i]) for i, k in enumerate(WIDE)}
    return rows, own


def narrow(lib, group, cnt, n):
    return call(lib.t_narrow, NARROW, group, C.c_uint64(cnt), C.c_uint32(n))


SORT_BASE = 1 << 40


def narrow_bare(lib, group, tables, n, is_sorted):
    return call(lib.t_narrow_bare, NARROW, group, C.c_uint64(tables), C.c_uint32(n), int(is_sorted), C.c_uint64(SORT_BASE))


# ---- the arrays' extents, from the shapes the kernels index them by -----------------------------------------------------------------
def msm_max_items(n, bare):
    return 573504 if not bare and n > 1 << 18 else 131072


def dense_extents(rows, n, bare, bw):
    mi = msm_max_items(n, bare)
    e = {k: rows * B16 * 4 for k in ("counts", "offsets", "order", "item_first")}
    e.update(item_count=rows * 16, ones_count=rows * 16, items=rows * mi * 8, buckets=rows * B16 * bw * 4, partial=rows * 4096 * bw * 4,
             partial_items=rows * mi * bw * 4, entries=rows * (n if bare else 16 * n) * 4, ones_list=rows * (0 if bare else n) * 4)
    if bare:
        e.update(digits=16 * n * 2, window_sums=16 * bw * 4)
    return e


def narrow_params(n):
    target = min(max((n // 128 + 2047) // 2048 * 2048, 2048), 65536)
    return dict(target=target, max_items=target + 256, ones_stride=(65536 if n > 1 << 18 else 4096) // 64, slices=128 if n > 1 << 18 else 16)


def narrow_extents(cnt, n, bw):
    p = narrow_params(n)
    e = dict(slice_hist=cnt * p["slices"] * B8 * 4, counts=cnt * B8 * 4, offsets=cnt * B8 * 4, item_first=cnt * B8 * 4, items=cnt * p["max_items"] * 4,
             item_count=cnt * 16, ones_count=cnt * 16, ones_list=cnt * n * 4, entries=cnt * 32 * n * 4, partial_items=cnt * p["max_items"] * bw * 4,
             partial_ones=cnt * p["ones_stride"] * bw * 4, folded_ones=cnt * 64 * bw * 4 if p["ones_stride"] > 64 else 0, bucket_sums=cnt * B8 * bw * 4)
    return e


def narrow_bare_extents(tables, n, bw, is_sorted):
    p = narrow_params(n)
    e = dict(partial_items=tables * 32 * p["max_items"] * bw * 4, partial_ones=tables * p["ones_stride"] * bw * 4, folded_ones=tables * 64 * bw * 4,
             bucket_sums=tables * 32 * B8 * bw * 4, window_sums=tables * 32 * bw * 4)
    if not is_sorted:
        e.update(entry_base=32 * 8, slice_hist=32 * p["slices"] * B8 * 4, counts=32 * B8 * 4, offsets=32 * B8 * 4, item_first=32 * B8 * 4,
                 items=32 * p["max_items"] * 4, item_count=32 * 16, ones_count=16, ones_list=n * 4, entries=32 * n * 4)
    return e


def check_arrays(offsets, extents, size, aligned16=(), aligned8=()):
    """inside [0, size), pairwise disjoint, aligned"""
    spans = sorted((offsets[k], offsets[k] + extents[k], k) for k in extents)
    for lo, hi, k in spans:
        assert 0 <= lo and hi <= size, (k, lo, hi, size)
    for (_, hi, a), (lo, _, b) in zip(spans, spans[1:]):
        assert hi <= lo, (a, b, hi, lo)
    for k in aligned16:
        assert offsets[k] % 16 == 0, k
    for k in aligned8:
        assert offsets[k] % 8 == 0, k


# ---- the four MSM layouts against the parent commit's ---------------------------------------------------------------------------------
def test_golden_file_names_its_origin(golden):
    assert len(golden["parent_commit"]) == 40
    s = golden["shapes"]
    assert s["n"] == NS and s["dense_rows"] == [1, 3, 17] and s["wide_n"] == [300, 1 << 18] and s["narrow_cnt"] == [1, 3, 17, 65]
    assert s["narrow_bare_tables"] == [1, 2, 3] and s["narrow_bare_sorted"] == [False, True] and s["group"] == [1, 2]
    cases = golden["cases"]
    count = {k: sum(c["layout"] == k for c in cases) for k in ("dense", "wide", "narrow", "narrow_bare")}
    assert count == {"dense": 6 * 3 * 2 * 2, "wide": 2 * 2, "narrow": 6 * 4 * 2, "narrow_bare": 6 * 3 * 2 * 2}


def test_dense_layout(lib, golden):
    cases = [c for c in golden["cases"] if c["layout"] == "dense"]
    for c in cases:
        g, rows, n, bare, bw = c["group"], c["rows"], c["n"], c["bare"], BW[c["group"]]
        got = dense(lib, g, rows, n, bare)
        for k, v in c["offsets"].items():
            assert got[k] == v, (c, k)
        assert (got["max_items"], got["ent_stride"], got["ones_stride"]) == (c["max_items"], c["ent_stride"], c["ones_stride"])
        assert ("digits" in got) == bare and ("window_sums" in got) == bare
        ext = dense_extents(rows, n, bare, bw)
        check_arrays(got, ext, got["bytes"], aligned16=["counts", "offsets", "order", "item_first", "item_count", "ones_count", "items", "buckets", "partial",
                                                        "partial_items", "entries"] + (["window_sums"] if bare else []))
        assert got["bytes"] % 16 == 0 and got["end"] <= got["bytes"]
        # the borrowings: the slices' histograms in the buckets, a lone row's 224 in its work items' partial sums
        assert rows * 32 * B16 * 4 <= ext["buckets"] and 224 * B16 * 4 <= dense_extents(1, n, bare, bw)["partial_items"]


def test_wide_layout(lib, golden):
    R, BINS = 208, 13 * 512
    for c in (c for c in golden["cases"] if c["layout"] == "wide"):
        g, n, bw = c["group"], c["n"], BW[c["group"]]
        rows, own = wide(lib, g, n)
        exp = c["offsets"]
        for k in ("counts", "offsets", "order", "item_first", "item_count", "ones_count", "items", "buckets", "partial", "partial_items"):
            assert rows[k] == exp[k], (c, k)
        assert (rows["entries"], rows["ones_list"], rows["end"]) == (exp["rows_entries"], exp["rows_ones_list"], exp["rows_end"])
        for k in WIDE[:-1]:
            assert own[k] == exp[k], (c, k)
        assert rows["max_items"] == c["max_items"] == 65536 and own["bytes"] == a16(exp["end"])
        # the shared prefix is the dense layout's at 208 rows (up to the item list, which is half as long here)
        d = dense(lib, g, R, n, True)
        assert all(rows[k] == d[k] for k in ("counts", "offsets", "order", "item_first", "item_count", "ones_count", "items"))
        assert rows["partial"] - rows["buckets"] == d["partial"] - d["buckets"] and rows["buckets"] - rows["items"] == R * 65536 * 8
        ext = {k: v for k, v in dense_extents(R, n, True, bw).items() if k in ("counts", "offsets", "order", "item_first", "item_count", "ones_count", "buckets", "partial")}
        ext.update(items=R * 65536 * 8, partial_items=R * 65536 * bw * 4, partial_plain=R * 4096 * bw * 4, s1=R * bw * 4, s0=R * bw * 4, window_sums=13 * bw * 4,
                   row_start=R * 8, bin_start=BINS * 8, row_count=R * 4, bin_count=BINS * 4, slice_hist=13 * 128 * 512 * 4, coarse=13 * n * 8, entries=13 * n * 4)
        offs = dict(rows)
        offs.update(own)
        offs["partial_items"] = rows["partial_items"]
        check_arrays(offs, ext, own["bytes"], aligned16=[k for k in ext if k not in ("entries",)], aligned8=["row_start", "bin_start", "coarse"])
        # the borrowings: the digits over the entries, the parts' histograms in the buckets
        assert own["digits"] == own["entries"] and BINS * 32 * 1024 * 4 <= ext["buckets"]


def test_narrow_layout(lib, golden):
    cases = [c for c in golden["cases"] if c["layout"] == "narrow"]
    assert any(c["cnt"] == 65 and c["ones_stride"] > 64 for c in cases)
    for c in cases:
        g, cnt, n, bw = c["group"], c["cnt"], c["n"], BW[c["group"]]
        got = narrow(lib, g, cnt, n)
        for k, v in c["offsets"].items():
            assert got[k] == v, (c, k)
        assert (got["target"], got["max_items"], got["ones_stride"]) == (c["target"], c["max_items"], c["ones_stride"])
        assert got["used"] == got["end"] and "entry_base" not in got and "window_sums" not in got
        check_arrays(got, narrow_extents(cnt, n, bw), got["used"],
                     aligned16=["slice_hist", "counts", "offsets", "item_first", "items", "item_count", "ones_count", "ones_list", "partial_items", "partial_ones",
                                "folded_ones", "bucket_sums"])
        # what a caller is told for `cnt` signatures holds the layout of `cnt`
        one = narrow(lib, g, 1, n)
        assert one["bytes"] == a16(one["used"] + 16) and got["used"] <= cnt * one["bytes"]


def test_narrow_bare_layout(lib, golden):
    for c in (c for c in golden["cases"] if c["layout"] == "narrow_bare"):
        g, tables, n, is_sorted, bw = c["group"], c["tables"], c["n"], c["sorted"], BW[c["group"]]
        got = narrow_bare(lib, g, tables, n, is_sorted)
        for k, v in c["offsets"].items():
            assert got[k] == v, (c, k)
        assert (got["target"], got["max_items"], got["ones_stride"], got["sort_n"]) == (c["target"], c["max_items"], c["ones_stride"], c["sort_n"])
        assert got["used"] == got["end"]
        ext = narrow_bare_extents(tables, n, bw, is_sorted)
        check_arrays(got, ext, got["used"], aligned16=[k for k in ext if k != "entries"], aligned8=["entry_base"] if not is_sorted else [])
        if is_sorted:
            # the sort's arrays are the other layout's, untouched
            other = narrow_bare(lib, 1, 1, n, False)
            for k in ("entry_base", "slice_hist", "counts", "offsets", "item_first", "items", "item_count", "ones_count", "ones_list", "entries"):
                assert got[k] == SORT_BASE + other[k], k


def test_sizes_reported_per_signature(lib, golden):
    rows = golden["per_signature"]
    assert sorted((r["n"], r["group"]) for r in rows) == sorted(itertools.product(NS, (1, 2)))
    for r in rows:
        out = (C.c_uint64 * 5)()
        lib.t_per_signature(r["group"], C.c_uint32(r["n"]), out)
        assert [int(x) for x in out] == [r["dense"], r["dense_bare"], r["dense_wide"], r["narrow"], r["narrow_bare"]], r
        assert dense(lib, r["group"], 16, r["n"], True)["window_sums"] == r["dense_bare_window_sums"]


# ---- the prover's layouts ---------------------------------------------------------------------------------------------------------------
def test_points_block(lib):
    assert lib.t_points_bytes() == 6 * 240 + 192 + 64 + 64
    for cnt in (1, 2, 5, 64):
        out = (C.c_uint64 * 9)()
        assert lib.t_points(C.c_uint64(cnt), out) == cnt * (6 * 240 + 192 + 64 + 64)
        p = dict(zip(POINTS, (int(x) for x in out)))
        # [A | B1' | L] [H] [s A | r B1'] B2 rs split, `cnt` of each
        exp, at = {}, 0
        for k, size in zip(POINTS, [240] * 6 + [192, 64, 64]):
            exp[k] = at
            at += cnt * size
        assert p == exp
        assert all(p[k] % 8 == 0 for k in ("B2", "rs", "split"))


PROVER_MSM = [[1177808, 1000, 256, 4097, 36792256], [512, 768, 1024, 1280, 1536]]         # bytes per signature: not / all multiples of 256


@pytest.mark.parametrize("cnt", [1, 2, 5, 64])
@pytest.mark.parametrize("msm", PROVER_MSM)
def test_table_prover_layout(lib, cnt, msm):
    qap, domain, nv = 123456, 4096, 2317
    out = (C.c_uint64 * 17)()
    size = lib.t_groth16(*u64(cnt, qap, domain, nv), (C.c_uint64 * 5)(*msm), out)
    points = 6 * 240 + 192 + 64 + 64
    per = a256(qap + 32 * domain + 32 * (nv + 3) + sum(a256(m) for m in msm) + points)
    if cnt == 1:
        assert size == per
    assert size <= cnt * per
    exp, at = [], 0
    for piece in [qap, 32 * domain, 32 * (nv + 3)] + [a256(m) for m in msm]:
        exp.append(at)
        at += cnt * piece
    assert [int(x) for x in out[:8]] == exp
    assert int(out[8]) == at and int(out[16]) + cnt * 64 == at + cnt * points <= size
    assert int(out[1]) % 8 == 0 and int(out[2]) % 8 == 0


@pytest.mark.parametrize("qap,msm_h", [(1000, 70000), (70001, 1000)])
@pytest.mark.parametrize("nz,b_rows", [(300, 5), ((1 << 18) + 1, 63)])
def test_bare_prover_layout(lib, qap, msm_h, nz, b_rows):
    domain, nv = 1 << 12, 2317
    out = (C.c_uint64 * 19)()
    size = lib.t_groth16_bare(*u64(qap, msm_h, domain, nv), C.c_uint32(nz), C.c_uint32(b_rows), out)
    msm_1 = a256(narrow_bare(lib, 1, 2, nz, False)["used"])
    msm_2 = a256(narrow_bare(lib, 1, 1, b_rows, False)["used"])
    msm_4 = a256(narrow_bare(lib, 2, 1, b_rows, True)["used"])
    points = 6 * 240 + 192 + 64 + 64
    assert size == a256(max(a256(msm_h), a256(qap)) + 32 * domain + 32 * (nv + 3) + msm_1 + msm_2 + msm_4 + points)
    first = max(a256(msm_h), a256(qap))
    g1 = first + 32 * domain + 32 * (nv + 3)
    assert [int(x) for x in out[:6]] == [0, first, first + 32 * domain, g1, g1 + msm_1, g1 + msm_1 + msm_2]
    assert int(out[6]) == g1 + msm_1 + msm_2 + msm_4 and int(out[14]) + 64 == int(out[6]) + points <= size
    assert [a256(int(x)) for x in out[15:18]] == [msm_1, msm_2, msm_4] and int(out[18]) == 1


# ---- the verification chains ------------------------------------------------------------------------------------------------------------
CHAINS = [dict(proof=0, pas=0, wire=0), dict(proof=21504, pas=4608, wire=0), dict(proof=21504, pas=4608, wire=1)]


def chain_size(k, msm_per, bare, proof, pas, wire):
    verify = msm_per * (1 if bare else k) + 96 * k + a16(4 * k)
    full = verify + k * proof + pas
    return (384 * k + a16(4 * k) if wire else 0) + full


@pytest.mark.parametrize("k", [1, 2, 5, 64])
@pytest.mark.parametrize("msm_per", [1177808, 36792320])                    # a multiple of 16 only, and one of 256
@pytest.mark.parametrize("bare", [0, 1])
@pytest.mark.parametrize("chain", CHAINS)
def test_verify_layouts(lib, k, msm_per, bare, chain):
    proof, pas, wire = chain["proof"], chain["pas"], chain["wire"]
    out = (C.c_uint64 * 7)()
    size = lib.t_verify(*u64(k, msm_per), bare, *u64(proof, pas), wire, out)
    assert size == chain_size(k, msm_per, bare, proof, pas, wire)
    v = [int(x) for x in out]
    front = 384 * k + a16(4 * k) if wire else 0
    m = msm_per * (1 if bare else k)
    assert v[2:] == [front, front + m, front + m + 96 * k, front + m + 96 * k + a16(4 * k), m]
    assert (v[0], v[1]) == ((0, 384 * k) if wire else (ABSENT, ABSENT))
    assert v[3] % 8 == 0 and v[5] % 16 == 0 and v[5] + k * proof + pas == size


@pytest.mark.parametrize("msm_per", [1177808, 36792320])
@pytest.mark.parametrize("bare", [0, 1])
@pytest.mark.parametrize("chain", CHAINS)
def test_proofs_in_flight(lib, msm_per, bare, chain):
    proof, pas, wire = chain["proof"], chain["pas"], chain["wire"]

    def size(k):
        return chain_size(k, msm_per, bare, proof, pas, wire)

    def fit(batch, budget):
        return lib.t_in_flight(*u64(batch, budget, msm_per), bare, *u64(proof, pas), wire)

    for k in (1, 2, 5, 64):
        assert fit(1000, size(k)) == k
        assert fit(1000, size(k) - 1) == k - 1
        assert fit(k, size(1000)) == k                     # never more than the batch
    assert fit(1000, size(1) - 1) == 0 and fit(0, size(5)) == 0
