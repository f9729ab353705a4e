"""The compiler's resource report for the witness map of the domains below 2^14 (falcon-r1cs_amd/csrc/frw_qap_small.hip; hipcc
cross-compiles gfx950 without a GPU): both kernels exist in both forms, none of them uses scratch memory, and their LDS is what
DESIGN 5.12 states -- 131,072 bytes (4,096 packed elements, the 2^12 domain's array) where the array stays in LDS, none where the 2^13
domain's stages go through the workspace.  Resource metadata only; no instruction is looked at."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# kernel -> LDS bytes per workgroup
KERNELS = {"frw::qap_small_coset_kernel<false>(": 131072, "frw::qap_small_h_kernel<false>(": 131072,
           "frw::qap_small_coset_kernel<true>(": 0, "frw::qap_small_h_kernel<true>(": 0}


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_the_small_domain_kernels_compile_without_scratch():
    import kernel_resources as KR
    rows = KR.compile_report(os.path.join(KR.CSRC, "frw_qap_small.hip"))
    assert len(rows) == len(KERNELS), [k["name"] for k in rows]
    for name, lds in KERNELS.items():
        hit = [k for k in rows if k["name"].startswith(name)]
        assert len(hit) == 1, (name, [k["name"] for k in rows])
        print(KR.fmt("frw_qap_small.hip", hit[0]))
        assert hit[0]["scratch"] == 0, KR.fmt("frw_qap_small.hip", hit[0])
        assert hit[0]["lds"] == lds, KR.fmt("frw_qap_small.hip", hit[0])
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "131,072 bytes" in design.split("### 5.12")[-1], "DESIGN 5.12 does not state the kernels' LDS"
