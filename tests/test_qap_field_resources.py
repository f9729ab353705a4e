"""The compiler's resource report for the kernels of the witness map over a run-time modulus (falcon-r1cs_amd/csrc/frw_qap_field.hip;
hipcc cross-compiles gfx950 without a GPU): none of them may use scratch memory -- the limbs of an element and the nine-limb accumulator
of a CIOS round are indexed with compile-time indices only -- and each reaches the waves per SIMD tools/kernel_resources.py lists for
it.  Resource metadata only; no instruction is looked at."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_the_field_map_kernels_compile_without_scratch_at_their_occupancy():
    import kernel_resources as KR
    listed = KR.HOT_WHOLE["frw_qap_field.hip"]
    assert sorted(listed) == ["frw::qapf_pass_kernel<11>", "frw::qapf_pass_kernel<12>"]
    rows = KR.compile_report(os.path.join(KR.CSRC, "frw_qap_field.hip"))
    assert len(rows) == len(listed), [k["name"] for k in rows]                 # every kernel of the unit is on the list
    for name, (scratch_ok, waves_min) in listed.items():
        hit = [k for k in rows if k["name"].startswith(name + "(")]
        assert len(hit) == 1, (name, [k["name"] for k in rows])
        print(KR.fmt("frw_qap_field.hip", hit[0]))
        assert scratch_ok == 0 and hit[0]["scratch"] == 0, KR.fmt("frw_qap_field.hip", hit[0])
        assert hit[0]["waves"] >= waves_min, KR.fmt("frw_qap_field.hip", hit[0])
        assert hit[0]["lds"] == (32 << int(name[-3:-1])), KR.fmt("frw_qap_field.hip", hit[0])     # the tile: 8 limb planes of 2^LOG_TILE words
