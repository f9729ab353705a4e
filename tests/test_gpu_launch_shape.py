"""The launch shape a context reports (frw_diag_launch_shape, which bench.py holds its launches to) is the arithmetic of
falcon-r1cs_amd/csrc/frw_launch.h applied to that context's own CU count and to the residency it asked for the variant: for both
parameter sets, for the four encodings of the NTT witness kernel and for the batches at which verify_shape takes another branch.  No
kernel is launched.  The ten-line port of resident_grid / verify_shape below is held to the same table as tests/cpp/test_launch_host.cpp
(that test needs no GPU)."""
import pytest

import field_cases as F

PARTS, OVERSUB = 5, 4

# batch -> (grid, whole signatures) at 256 CUs for: 3 resident per CU, split | 3, no split | 4, split | 0 (falls back to 2), split
TABLE = {
    1: ((5, 0), (1, 1), (5, 0), (5, 0)),
    153: ((765, 0), (153, 153), (765, 0), (153, 153)),
    154: ((154, 154), (154, 154), (770, 0), (154, 154)),
    768: ((768, 768), (768, 768), (768, 768), (384, 768)),
    769: ((768, 768), (768, 769), (769, 769), (512, 512)),
    4096: ((2048, 4096), (2048, 4096), (2048, 4096), (2048, 4096)),
    8192: ((2048, 8192), (2048, 8192), (4096, 8192), (2048, 8192)),
    32768: ((3072, 30720), (3072, 32768), (4096, 32768), (2048, 32768)),
    100000: ((3072, 98304), (3072, 100000), (4096, 98304), (2048, 98304)),
}


def resident_grid(batch, num_cu, per_cu, oversub=OVERSUB):
    cap = (per_cu if per_cu > 0 else 2) * num_cu
    if batch <= cap:
        return batch
    top = min(oversub * cap, batch // 2) if batch >= 2 * cap else cap
    if batch < 8 * top:
        for g in range(top, (top * 5 + 7) // 8 - 1, -1):           # g * 8 >= top * 5
            if batch % g == 0:
                return g
    return top


def verify_shape(batch, num_cu, occ, may_split=True):
    cap = (occ if occ > 0 else 2) * num_cu
    if may_split and batch * PARTS <= cap:
        return batch * PARTS, 0
    grid = resident_grid(batch, num_cu, occ)
    return grid, (batch // grid * grid if may_split else batch)


def test_the_port_reproduces_the_table():
    for batch, row in TABLE.items():
        got = (verify_shape(batch, 256, 3), verify_shape(batch, 256, 3, False), verify_shape(batch, 256, 4), verify_shape(batch, 256, 0))
        assert got == row, (batch, got, row)
    assert [resident_grid(b, 256, 3, 8) for b in (1, 768, 4096, 8192, 32768, 65536)] == [1, 768, 2048, 4096, 4096, 6144]
    assert resident_grid(3072, 256, 2) == 1536 and verify_shape(100, 8, 2) == (50, 100)


@pytest.mark.gpu
def test_reported_shape_is_the_arithmetic_over_the_contexts_own_residency(engine):
    import falcon_r1cs_amd as frw
    field = engine.field_encoding(F.BN254)
    for logn in (9, 10):
        for enc in (frw.ENC_CANONICAL, frw.ENC_MONTGOMERY, frw.ENC_COMPACT, field):
            for batch in (1, 153, 154, 768, 769, 8192, 32768):
                s = engine.launch_shape(logn, batch, enc)
                assert s["resident_per_cu"] >= 1 and s["cus"] >= 1, (logn, enc, batch, s)
                want = verify_shape(batch, s["cus"], s["resident_per_cu"])
                assert (s["grid"], batch - s["split_signatures"]) == want, (logn, enc, batch, s, want)
    # an encoding id this context did not hand out
    other = frw.WitnessEngine(0)
    try:
        for enc in (field, 3, -1, frw.ENC_FIELD_BASE + frw.MAX_FIELDS):
            with pytest.raises(frw.FrwError) as ei:
                other.launch_shape(10, 32768, enc)
            assert ei.value.code == -1                              # FRW_E_INVALID_ARG
    finally:
        other.close()
