"""The compiler's resource report for the routed preparation kernels of the aggregate from bytes (falcon-r1cs_amd/csrc/frw_prepare.hip;
hipcc cross-compiles gfx950 without a GPU): the routed hash, both routed decoders, the verdicts' scatter and the refused count exist
exactly once each and use no scratch memory; the kernels they share their bodies with are still there, once each, without scratch.
Resource metadata only; no instruction is looked at."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NEW = ["frw::agg_hash_to_point_kernel(", "frw::agg_decode_public_keys_kernel(", "frw::agg_decode_signatures_kernel(",
       "frw::agg_scatter_verdicts_kernel(", "frw::agg_count_refused_kernel("]
SHARED = ["frw::hash_to_point_kernel(", "frw::decode_public_keys_kernel(", "frw::decode_signatures_kernel("]


@pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")), reason="needs hipcc")
def test_the_routed_kernels_compile_once_each_without_scratch():
    import kernel_resources as KR
    rows = KR.compile_report(os.path.join(KR.CSRC, "frw_prepare.hip"))
    for name in NEW + SHARED:
        hit = [k for k in rows if k["name"].startswith(name)]
        assert len(hit) == 1, (name, [k["name"] for k in rows])
        print(KR.fmt("frw_prepare.hip", hit[0]))
        assert hit[0]["scratch"] == 0, KR.fmt("frw_prepare.hip", hit[0])
    # one lane per signature for the hash and the signature decoder: nothing of theirs is shared between lanes
    for name in NEW[:3]:
        assert [k for k in rows if k["name"].startswith(name)][0]["lds"] == 0, name
