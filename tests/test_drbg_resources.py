"""The compiler's resource report for the factor draw's kernels (falcon-r1cs_amd/csrc/frw_drbg.hip; hipcc cross-compiles gfx950 without a
GPU).  fr_draw_kernel holds a Keccak state of 25 words in a lane's registers, as the two existing users of the same permutation do
(hash_to_point, batch_scalar_kernel), and the 512-bit reduction beside it: no scratch memory, like them.  DESIGN.md 5.13 records the
register count this finds.  Only the resource metadata is read."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NS = "frw::drbg::(anonymous namespace)::"
KERNELS = ("fr_draw_kernel", "fr_draw_advance_kernel")


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_the_draw_kernels_have_no_scratch():
    import kernel_resources as KR
    assert "frw_drbg.hip" in KR.FILES
    rows = KR.compile_report(os.path.join(KR.CSRC, "frw_drbg.hip"))
    by_name = {}
    for name in KERNELS:
        hit = [k for k in rows if k["name"].startswith(NS + name + "(")]
        assert len(hit) == 1, (name, [k["name"] for k in rows])
        by_name[name] = hit[0]
        print(KR.fmt("frw_drbg.hip", hit[0]))
    assert len(rows) == len(KERNELS), [k["name"] for k in rows]
    for name in KERNELS:
        assert by_name[name]["scratch"] == 0 and by_name[name]["lds"] == 0 and by_name[name]["waves"] >= 1, KR.fmt("frw_drbg.hip", by_name[name])
    # DESIGN states the compiled figure
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 5.13"):]
    assert re.search(r"\b%d VGPRs" % by_name["fr_draw_kernel"]["vgpr"], section) and "no scratch" in section


def test_the_makefile_builds_the_unit():
    """the Makefile builds the unit and tracks the header"""
    mk = open(os.path.join(ROOT, "falcon-r1cs_amd", "csrc", "Makefile")).read()
    src = re.search(r"^SRC = (.*)$", mk, flags=re.M).group(1).split()
    hdr = re.search(r"^HDR = (.*)$", mk, flags=re.M).group(1).split()
    assert "frw_drbg.hip" in src and "frw_drbg.h" in hdr
