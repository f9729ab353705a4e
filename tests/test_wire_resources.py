"""The compiler's resource report for the wire codec's kernels (falcon-r1cs_amd/csrc/frw_wire.hip; hipcc cross-compiles gfx950 without a
GPU).  Decoding a compressed G1 point is one a^((q + 1) / 4): a square-and-multiply over ONE Fq29 accumulator with an exponent that is
the same constant in every lane -- nothing there needs scratch memory, so none is allowed.  The G2 kernel (two such roots, an
inversion, Fq2 arithmetic in one lane) and the encode kernel are reported (printed), not gated: profiles/r08_wire_kernel_resources.txt
has their figures."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PREFIX = "frw::wire::(anonymous namespace)::"
NO_SCRATCH = ["wire_g1_decode_kernel", "wire_g1_run_decode_kernel"]
REPORTED = ["wire_g2_decode_kernel", "wire_encode_proofs_kernel"]


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_g1_decoding_compiles_without_scratch():
    import kernel_resources as KR
    rows = KR.compile_report(os.path.join(KR.CSRC, "frw_wire.hip"))
    for name in NO_SCRATCH + REPORTED:
        hit = [k for k in rows if k["name"].startswith(PREFIX + name + "(")]
        assert len(hit) == 1, (name, [k["name"] for k in rows])
        print(KR.fmt("frw_wire.hip", hit[0]))
        if name in NO_SCRATCH:
            assert hit[0]["scratch"] == 0, KR.fmt("frw_wire.hip", hit[0])
