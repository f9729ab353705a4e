"""The compiler's resource report for the re-randomisation kernels (falcon-r1cs_amd/csrc/frw_rerand.hip; hipcc cross-compiles gfx950
without a GPU).  The two ladder kernels are where a re-randomisation spends its time: the G1 ladder keeps its addends in LDS and holds
ONE inlined addition, so that its points stay in registers (no scratch memory); the G2 ladder, two lanes per point, carries what the
existing two-lane G2 kernels carry (wire_run_subgroup_kernel<Fq2PairField> in profiles/r09_pk_wire_kernel_resources.txt: 688 bytes per
lane, one wave per SIMD), short of the target of none -- DESIGN.md 5.11 states the figure, and this test holds it so that it cannot grow.
`rerand_check_kernel` runs the same
two-lane subgroup ladder and is held to the same figure.  Only the resource metadata is read."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NS = "frw::rerand::(anonymous namespace)::"
KERNELS = ("rerand_check_kernel", "rerand_factor_kernel", "rerand_g1_kernel", "rerand_g2_kernel", "rerand_finish_kernel<frw::FqField>",
           "rerand_finish_kernel<frw::Fq2PairField>", "rerand_wire_clear_kernel")
G2_SCRATCH, G2_WAVES = 688, 1
CHECK_SCRATCH, CHECK_WAVES = 688, 1       # rerand_check_kernel: the same two-lane G2 subgroup ladder, 37 % of a checked call


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_the_ladder_kernels_resources():
    import kernel_resources as KR
    rows = KR.compile_report(os.path.join(KR.CSRC, "frw_rerand.hip"))
    by_name = {}
    for name in KERNELS:
        hit = [k for k in rows if k["name"].startswith(NS + name + "(")]
        assert len(hit) == 1, (name, [k["name"] for k in rows])
        by_name[name] = hit[0]
    g1, g2 = by_name["rerand_g1_kernel"], by_name["rerand_g2_kernel"]
    assert g1["scratch"] == 0 and g1["waves"] >= 1, KR.fmt("frw_rerand.hip", g1)
    assert g2["scratch"] <= G2_SCRATCH and g2["waves"] >= G2_WAVES, KR.fmt("frw_rerand.hip", g2)
    chk = by_name["rerand_check_kernel"]
    assert chk["scratch"] <= CHECK_SCRATCH and chk["waves"] >= CHECK_WAVES, KR.fmt("frw_rerand.hip", chk)
    # no more than the existing two-lane G2 kernels carry, by the committed report
    report = open(os.path.join(ROOT, "profiles", "r09_pk_wire_kernel_resources.txt")).read()
    row = next(l for l in report.splitlines() if "wire_run_subgroup_kernel<frw::Fq2PairField>" in l)
    assert g2["scratch"] <= int(row.split()[4])
    assert chk["scratch"] <= int(row.split()[4])
    # the finish (an inversion per point) and the factors' integer arithmetic spill nothing
    for name in ("rerand_factor_kernel", "rerand_finish_kernel<frw::FqField>", "rerand_finish_kernel<frw::Fq2PairField>", "rerand_wire_clear_kernel"):
        assert by_name[name]["scratch"] == 0, KR.fmt("frw_rerand.hip", by_name[name])
    # DESIGN states the compiled figures
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 5.11"):]
    assert re.search(r"%d bytes" % G2_SCRATCH, section) and "no scratch" in section
