"""The compiler's resource report for the Falcon verification kernel (falcon-r1cs_amd/csrc/frw_kernels.hip; hipcc cross-compiles
gfx950 without a GPU): none of its four instantiations (logn x rule) may use scratch memory, and its LDS -- the twiddles and four
uint16_t[N] arrays -- stays at a third of the witness kernel's, so the wave cap and not LDS limits residency.  Resource metadata only;
no instruction is looked at."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ["frw::falcon_verify_kernel<%d, %d>(" % (logn, rule) for logn in (9, 10) for rule in (0, 1)]


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_the_falcon_verify_kernel_compiles_without_scratch():
    import kernel_resources as KR
    rows = KR.compile_report(os.path.join(KR.CSRC, "frw_kernels.hip"))
    for name in KERNELS:
        hit = [k for k in rows if k["name"].startswith(name)]
        assert len(hit) == 1, (name, [k["name"] for k in rows])
        print(KR.fmt("frw_kernels.hip", hit[0]))
        assert hit[0]["scratch"] == 0, KR.fmt("frw_kernels.hip", hit[0])
        # twiddles + sig, its transform, pk, hm (10 N bytes) + the norm and two status words: 10.3 KB at N = 1024
        assert hit[0]["lds"] <= 16384, KR.fmt("frw_kernels.hip", hit[0])
