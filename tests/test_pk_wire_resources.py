"""The compiler's resource report for the proving-key kernels of the wire codec (falcon-r1cs_amd/csrc/frw_wire.hip; hipcc cross-compiles
gfx950 without a GPU).  The G1 kernels -- the run decoder (one square root over one accumulator), the subgroup ladder over one XYZZ
accumulator and the row encoder -- have nothing that needs scratch memory, the condition the proof decoder's G1 kernel already meets, so
none is allowed.  The G2 kernels (Fq2 in one lane for the decoder and the encoder, the two-lane Fq2 for the ladder) are reported
(printed), not gated: profiles/r09_pk_wire_kernel_resources.txt has their figures, and no earlier figure exists to cap them by.
Resource metadata only; no instruction is looked at."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PREFIX = "frw::wire::(anonymous namespace)::"
NO_SCRATCH = ["wire_g1_run_decode_kernel(", "wire_run_subgroup_kernel<frw::FqField>(", "wire_rows_encode_kernel<frw::FqField>("]
REPORTED = ["wire_g2_run_decode_kernel(", "wire_run_subgroup_kernel<frw::Fq2PairField>(", "wire_rows_encode_kernel<frw::Fq2Field>("]


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_the_g1_kernels_of_a_key_compile_without_scratch():
    import kernel_resources as KR
    rows = KR.compile_report(os.path.join(KR.CSRC, "frw_wire.hip"))
    for name in NO_SCRATCH + REPORTED:
        hit = [k for k in rows if k["name"].startswith(PREFIX + name)]
        assert len(hit) == 1, (name, [k["name"] for k in rows])
        print(KR.fmt("frw_wire.hip", hit[0]))
        if name in NO_SCRATCH:
            assert hit[0]["scratch"] == 0, KR.fmt("frw_wire.hip", hit[0])
