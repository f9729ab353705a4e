"""The compiler's resource report for the schoolbook witness kernel (falcon-r1cs_amd/csrc/frw_kernels.hip; hipcc cross-compiles
gfx950 without a GPU): none of its four instantiations may use scratch memory.  Resource metadata only; no instruction is
looked at."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ["frw::witness_schoolbook_verify_kernel<%d, %d>(" % (logn, enc) for logn in (9, 10) for enc in (0, 1)]


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_the_schoolbook_kernel_compiles_without_scratch():
    import kernel_resources as KR
    rows = KR.compile_report(os.path.join(KR.CSRC, "frw_kernels.hip"))
    for name in KERNELS:
        hit = [k for k in rows if k["name"].startswith(name)]
        assert len(hit) == 1, (name, [k["name"] for k in rows])
        print(KR.fmt("frw_kernels.hip", hit[0]))
        assert hit[0]["scratch"] == 0, KR.fmt("frw_kernels.hip", hit[0])
