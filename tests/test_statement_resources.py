"""The compiler's resource report for the statement kernel (falcon-r1cs_amd/csrc/frw_kernels.hip; hipcc cross-compiles gfx950
without a GPU): none of its eight instantiations (logn x form x encoding) may use scratch memory, and its LDS stays far under the
witness kernel's 50 KB.  Resource metadata only; no instruction is looked at."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ["frw::statement_kernel<%d, %d, %d>(" % (logn, form, enc) for logn in (9, 10) for form in (0, 1) for enc in (0, 1)]


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_the_statement_kernel_compiles_without_scratch():
    import kernel_resources as KR
    rows = KR.compile_report(os.path.join(KR.CSRC, "frw_kernels.hip"))
    for name in KERNELS:
        hit = [k for k in rows if k["name"].startswith(name)]
        assert len(hit) == 1, (name, [k["name"] for k in rows])
        print(KR.fmt("frw_kernels.hip", hit[0]))
        assert hit[0]["scratch"] == 0, KR.fmt("frw_kernels.hip", hit[0])
        # slab (8,704) + twiddles and one polynomial (4 N) + the verdict: 12.8 KB at N = 1024
        assert hit[0]["lds"] <= 16384, KR.fmt("frw_kernels.hip", hit[0])
