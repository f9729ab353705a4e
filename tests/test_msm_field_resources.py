"""The compiler's resource report for the kernels of the sum over a run-time curve (falcon-r1cs_amd/csrc/frw_msm_field.hip; hipcc
cross-compiles gfx950 without a GPU): every kernel of the unit is on tools/kernel_resources.py's list, none of them uses scratch memory
-- the limbs of a coordinate and the nine-limb accumulator of a CIOS round are indexed with compile-time indices only, and an XYZZ
accumulator, a point and a mixed addition's temporaries fit the registers of four waves per SIMD -- and each reaches the waves per SIMD
listed for it.  Resource metadata only; no instruction is looked at."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_the_curve_sum_kernels_compile_without_scratch_at_their_occupancy():
    import kernel_resources as KR
    listed = KR.HOT_WHOLE["frw_msm_field.hip"]
    assert sorted(listed) == ["frw::msmf_bucket_kernel", "frw::msmf_check_kernel", "frw::msmf_clear_kernel", "frw::msmf_digits_kernel<13, 20>", "frw::msmf_digits_kernel<15, 18>",
                              "frw::msmf_finish_kernel", "frw::msmf_fold_kernel", "frw::msmf_scan_kernel", "frw::msmf_scatter_kernel"]
    assert listed["frw::msmf_bucket_kernel"] == (0, 4)
    rows = KR.compile_report(os.path.join(KR.CSRC, "frw_msm_field.hip"))
    assert len(rows) == len(listed), [k["name"] for k in rows]                 # every kernel of the unit is on the list
    for name, (scratch_ok, waves_min) in listed.items():
        hit = [k for k in rows if k["name"].startswith(name + "(")]
        assert len(hit) == 1, (name, [k["name"] for k in rows])
        print(KR.fmt("frw_msm_field.hip", hit[0]))
        assert scratch_ok == 0 and hit[0]["scratch"] == 0, KR.fmt("frw_msm_field.hip", hit[0])
        assert hit[0]["waves"] >= waves_min, KR.fmt("frw_msm_field.hip", hit[0])
