"""The compiler's resource report for the compaction kernels of the prover from bytes (falcon-r1cs_amd/csrc/frw_prepare.hip; hipcc
cross-compiles gfx950 without a GPU): the three scan passes, both gathers, the zero fill and the scatter exist, use no scratch memory
and next to no LDS (the scan's per-wavefront counts).  Resource metadata only; no instruction is looked at."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ["frw::pok_scan_count_kernel(", "frw::pok_scan_offsets_kernel(", "frw::pok_scan_write_kernel(", "frw::pok_gather_rs_kernel(",
           "frw::pok_gather_inputs_kernel(", "frw::pok_zero_refused_kernel(", "frw::pok_scatter_kernel("]


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_the_compaction_kernels_compile_without_scratch():
    import kernel_resources as KR
    rows = KR.compile_report(os.path.join(KR.CSRC, "frw_prepare.hip"))
    for name in KERNELS:
        hit = [k for k in rows if k["name"].startswith(name)]
        assert len(hit) == 1, (name, [k["name"] for k in rows])
        print(KR.fmt("frw_prepare.hip", hit[0]))
        assert hit[0]["scratch"] == 0, KR.fmt("frw_prepare.hip", hit[0])
        assert hit[0]["lds"] <= 64, KR.fmt("frw_prepare.hip", hit[0])          # four words per scan pass, none elsewhere
