"""The compiler's resource report for the device pairing's kernels (falcon-r1cs_amd/csrc/frw_pairing_dev.hip, hipcc cross-compiles
gfx950 without a GPU): the Miller loop and the final exponentiation's chain of z-powers -- where a device verification spends its
time -- hold an Fq12 across eight lanes so that they run two waves per SIMD with little or no scratch memory.  A one-lane-per-pairing port
of frw_pairing.h needs 15 KB of scratch per lane; this test notices if the kernels drift back towards it."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# kernel name prefix -> (scratch bytes per lane allowed, waves per SIMD at least).  The Miller loop meets the target, no scratch and two
# waves.  The hard part of the final exponentiation runs two waves (Granger - Scott squarings, products through LDS) but the compiler
# still spills 152 bytes per lane there; the bound holds that figure so that it cannot grow, short of the target of none.
HOT = {"frw::pairing_dev::(anonymous namespace)::miller_kernel": (0, 2),
       "frw::pairing_dev::(anonymous namespace)::final_exp_hard_kernel": (152, 2)}


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_miller_loop_and_final_exponentiation_run_two_waves_without_growing_scratch():
    import kernel_resources as KR
    rows = KR.compile_report(os.path.join(KR.CSRC, "frw_pairing_dev.hip"))
    for prefix, (scratch_ok, waves_min) in HOT.items():
        hit = [k for k in rows if k["name"].startswith(prefix)]
        assert len(hit) == 1, (prefix, [k["name"] for k in rows])
        k = hit[0]
        assert k["scratch"] <= scratch_ok and k["waves"] >= waves_min, KR.fmt("frw_pairing_dev.hip", k)
