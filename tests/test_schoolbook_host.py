"""The schoolbook circuit without a GPU: frw_layout_schoolbook's counts and frw_r1cs_export(FRW_CIRCUIT_SCHOOLBOOK, ...)
against the ORACLE's FalconSchoolBookVerificationCircuit (oracle/falcon_gadgets.py on oracle/ark_sim.py): identical
matrices entry by entry at N = 512, satisfied by the oracle's witness and by no tampered one."""
import ctypes as C

import numpy as np
import pytest

import schoolbook_ref as S
from test_r1cs_export import export, read_r1cs

P = S.P
# README.md:45,56 of the reference: variables (witness), constraints
README_COUNTS = {9: (312882, 315956), 10: (1150004, 1156150)}


@pytest.mark.parametrize("logn", [9, 10])
def test_layout_reproduces_the_published_counts(logn):
    import falcon_r1cs_amd as frw
    L = frw.layout_schoolbook(logn)
    n = 1 << logn
    assert (L.num_witness, L.num_constraints) == README_COUNTS[logn]
    assert (L.num_instance, L.num_witness, L.num_constraints) == S.counts(logn)
    assert L.num_instance == 2 * n + 1 and L.column_len == n + 34 and (L.logn, L.n) == (logn, n)
    assert L.seg_len == (n, 28 * n, n * (n + 34), 36 * n, 50 if logn == 9 else 52)
    assert L.seg_off == (0, n, 29 * n, n * n + 63 * n, n * n + 99 * n)
    assert L.seg_off[-1] + L.seg_len[-1] == L.num_witness
    assert all(L.seg_off[i] + L.seg_len[i] == L.seg_off[i + 1] for i in range(4))
    assert (L.column_len * 32) % 64 == 0 and (L.seg_off[2] * 32) % 64 == 0      # every column starts 64-byte aligned


def test_layout_and_entry_points_refuse_what_they_do_not_serve():
    import falcon_r1cs_amd as frw
    from falcon_r1cs_amd._lib import LayoutSchoolbookStruct
    lib = frw.load_library()
    s = LayoutSchoolbookStruct()
    for logn in (8, 11, 0, -1):
        assert lib.frw_layout_schoolbook(logn, C.byref(s)) == -1
    assert lib.frw_layout_schoolbook(9, None) == -1
    assert lib.frw_r1cs_export(3, 9, b"/dev/null", None) == -1                    # unknown circuit id
    assert lib.frw_r1cs_export(S.CIRCUIT_SCHOOLBOOK, 8, b"/dev/null", None) == -1
    # no context: invalid argument before any device is touched (FRW_ENC_COMPACT is refused the same way with one)
    assert lib.frw_witness_schoolbook_verify_dev(None, 9, 1, None, None, None, 1, None, None, None, None) == -1
    assert lib.frw_witness_schoolbook_verify(None, 9, 1, None, None, None, 1, None, None, None, 0) == -1


@pytest.fixture(scope="module")
def exported(tmp_path_factory):
    path = tmp_path_factory.mktemp("schoolbook") / "c.r1cs"
    cnt = export(S.CIRCUIT_SCHOOLBOOK, 9, path)
    return cnt, read_r1cs(path)


def test_exported_header_and_matrices_equal_the_oracle(exported):
    cnt, (ni, nw, nc, mats) = exported
    cs = S.fixture_cs(9)
    assert (ni, nw, nc) == S.counts(9) == tuple(cnt[:3])
    assert (nw, nc) == README_COUNTS[9]
    assert (ni, nw, nc) == (cs.num_instance_variables(), cs.num_witness_variables(), cs.num_constraints())
    want = cs.to_matrices()
    for (ptr, col, val), rows in zip(mats, want):
        assert int(ptr[-1]) == sum(len(r) for r in rows)
        assert np.array_equal(col, np.fromiter((c for r in rows for c, _ in r), dtype=np.uint32))
        assert np.array_equal(np.diff(ptr.astype(np.int64)), np.fromiter((len(r) for r in rows), dtype=np.int64))
        assert val.tobytes() == b"".join(v.to_bytes(32, "little") for r in rows for _, v in r)
    # the shape the device-side evaluators meet: N^2 product rows of one term a side, N rows of N + 2 terms, few coefficients
    n = 512
    a_len = np.diff(mats[0][0].astype(np.int64))
    assert int((a_len == n + 2).sum()) == n and int((a_len == 1).sum()) >= n * n      # (the longest row is the norm's: 2 N + 26 terms)
    coefs = {bytes(v) for m in mats for v in m[2].view(np.uint8).reshape(-1, 32)}
    assert len(coefs) < 254


def _violated(mats, nc, z):
    prods = []
    for ptr, col, val in mats:
        vals = [int(a) | int(b) << 64 | int(c) << 128 | int(d) << 192 for a, b, c, d in val.tolist()]
        cols, p_ = col.tolist(), ptr.tolist()
        prods.append([sum(vals[k] * z[cols[k]] for k in range(p_[i], p_[i + 1])) % P for i in range(nc)])
    return sum(1 for a, b, c in zip(*prods) if (a * b - c) % P)


def test_oracle_witness_satisfies_the_export_and_tampered_ones_do_not(exported):
    _, (ni, nw, nc, mats) = exported
    cs = S.fixture_cs(9)
    assert cs.is_satisfied()
    n = 512
    z = list(cs.instance_assignment) + list(cs.witness_assignment)
    assert len(z) == ni + nw and _violated(mats, nc, z) == 0
    col7 = ni + 29 * n + 7 * (n + 34)                       # column 7 of B2
    # of a column's two multipliers only the one whose is_not_equal is 1 is bound (where the operands are equal the
    # difference is zero and AllocatedFp::is_neq leaves the multiplier free): that one is bumped
    mult = col7 + n + 30 if z[col7 + n + 29] == 1 else col7 + n + 32
    assert z[mult - 1] == 1 and z[mult] in (pow(S.Q, -1, P), pow(P - S.Q, -1, P))
    plant = {"a boolean of ltq(v[3])": ni + n + 3 * 28 + 2, "t of column 7": col7, "product 11 of column 7": col7 + 2 + 11,
             "the bound multiplier of column 7": mult}
    for what, idx in plant.items():
        bad = list(z)
        bad[idx] = (bad[idx] ^ 1) if "boolean" in what else (bad[idx] + 1) % P
        assert _violated(mats, nc, bad) > 0, what


def test_both_tails_occur_in_the_fixtures():
    for logn in (9,):
        lt, ge = S.tail_counts(S.fixture_cs(logn), logn)
        n = 1 << logn
        assert lt + ge == n and 10 * lt >= n and 10 * ge >= n, (lt, ge)
    for logn in (9, 10):                                    # and in the committed goldens (Falcon-1024 by its recorded counts)
        g = S.golden(logn)
        n = 1 << logn
        assert g["counts"] == dict(zip(("num_instance", "num_witness", "num_constraints"), S.counts(logn)))
        for t in g["triples"]:
            assert t["tails"]["hm_lt_c"] + t["tails"]["hm_ge_c"] == n and 10 * min(t["tails"].values()) >= n


def test_golden_512_is_what_the_oracle_gives():
    g = S.golden(9)
    cs = S.fixture_cs(9)
    sig, pk, hm = S.golden_triple(g, 0)
    assert all(np.array_equal(a, b) for a, b in zip((sig, pk, hm), S.triple(9, S.SEEDS[9][0])))
    for name, mont in (("canonical", False), ("montgomery", True)):
        wit, inst = S.encoded(cs, mont)
        assert g["triples"][0]["sha256"][name] == {"witness": S.sha(wit), "instance": S.sha(inst)}
