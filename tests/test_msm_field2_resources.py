"""The compiler's resource report for the kernels of the sum over a curve on a run-time Fq2 (falcon-r1cs_amd/csrc/frw_msm_field2.hip;
hipcc cross-compiles gfx950 without a GPU): every kernel of the unit is on tools/kernel_resources.py's list, the bucket kernel -- the hot
loop -- has no scratch at two waves per SIMD, no other kernel uses more scratch than its entry allows (none does: every XYZZ accumulator
over Fe2 is a column of LDS, not 64 registers), and each reaches the waves per SIMD listed for it.  Resource metadata only; no
instruction is looked at."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_the_fq2_curve_sum_kernels_compile_at_their_occupancy_and_the_bucket_kernel_without_scratch():
    import kernel_resources as KR
    unit = "frw_msm_field2.hip"
    listed = KR.HOT_WHOLE[unit]
    assert sorted(listed) == ["frw::msmf2_bucket_kernel", "frw::msmf2_check_kernel", "frw::msmf2_clear_kernel", "frw::msmf2_digits_kernel<13, 20>",
                              "frw::msmf2_digits_kernel<15, 18>", "frw::msmf2_finish_kernel", "frw::msmf2_fold_kernel", "frw::msmf2_scan_kernel",
                              "frw::msmf2_scatter_kernel"]
    assert listed["frw::msmf2_bucket_kernel"] == (0, 2)
    rows = KR.compile_report(os.path.join(KR.CSRC, unit))
    assert len(rows) == len(listed), [k["name"] for k in rows]                 # every kernel of the unit is on the list
    for name, (scratch_ok, waves_min) in listed.items():
        hit = [k for k in rows if k["name"].startswith(name + "(")]
        assert len(hit) == 1, (name, [k["name"] for k in rows])
        print(KR.fmt(unit, hit[0]))
        assert hit[0]["scratch"] <= scratch_ok, KR.fmt(unit, hit[0])
        assert hit[0]["waves"] >= waves_min, KR.fmt(unit, hit[0])
    bucket = [k for k in rows if k["name"].startswith("frw::msmf2_bucket_kernel(")][0]
    assert bucket["scratch"] == 0 and bucket["waves"] >= 2 and bucket["lds"] == 65536, KR.fmt(unit, bucket)
