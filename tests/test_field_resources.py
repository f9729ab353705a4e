"""The compiler's resource report for the run-time-field instantiations (ENC = 3) of falcon-r1cs_amd/csrc/frw_kernels.hip (hipcc
cross-compiles gfx950 without a GPU): none of them may use scratch memory -- the 33 words of constants are a by-value kernel argument,
not an indexed table --, and the witness kernel keeps the LDS size and the occupancy of its hard-wired Montgomery instantiation.
Resource metadata only; no instruction is looked at."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NEW = (["frw::witness_ntt_verify_kernel<%d, 3>(" % logn for logn in (9, 10)] +
       ["frw::ntt_modq_kernel<%d, 3>(" % logn for logn in (9, 10)] +
       ["frw::expand_kernel<%d, 3>(" % logn for logn in (9, 10)] +
       ["frw::gadget_kernel<%d, 3>(" % kind for kind in range(6)] +
       ["frw::statement_kernel<%d, %d, 3>(" % (logn, form) for logn in (9, 10) for form in (0, 1)])


@pytest.fixture(scope="module")
def rows():
    import kernel_resources as KR
    return KR, KR.compile_report(os.path.join(KR.CSRC, "frw_kernels.hip"))


def _one(rows, prefix):
    hit = [k for k in rows if k["name"].startswith(prefix)]
    assert len(hit) == 1, (prefix, [k["name"] for k in rows])
    return hit[0]


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_every_field_instantiation_compiles_without_scratch(rows):
    KR, report = rows
    assert len(NEW) == 16
    for name in NEW:
        k = _one(report, name)
        print(KR.fmt("frw_kernels.hip", k))
        assert k["scratch"] == 0, KR.fmt("frw_kernels.hip", k)


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
@pytest.mark.parametrize("logn", [9, 10])
def test_the_field_witness_kernel_keeps_lds_and_occupancy(rows, logn):
    KR, report = rows
    field = _one(report, "frw::witness_ntt_verify_kernel<%d, 3>(" % logn)
    wired = _one(report, "frw::witness_ntt_verify_kernel<%d, 1>(" % logn)
    print(KR.fmt("frw_kernels.hip", wired))
    print(KR.fmt("frw_kernels.hip", field))
    assert field["lds"] == wired["lds"]
    assert field["waves"] >= wired["waves"]
