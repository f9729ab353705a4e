"""The two rules of frw_falcon_verify* on the CPU, where they differ (tests/falcon_verify_cases.py builds the triples,
tests/test_gpu_falcon_verify.py runs the device on the same ones): FRW_RULE_CIRCUIT must be what the oracle's circuit
(oracle/falcon_gadgets.run_reference_flow) is satisfied by, FRW_RULE_SPEC what the specification's sum says."""
import numpy as np

import falcon_r1cs_amd as frw
import falcon_verify_cases as FV
from oracle import falcon_gadgets as G


def _satisfied(sig, pk, hm, logn):
    return G.run_reference_flow(sig.tolist(), pk.tolist(), hm.tolist(), logn, strict=False).is_satisfied()


def test_the_circuit_is_satisfied_below_the_bound_and_not_at_it():
    """Falcon-512 triples of four non-zero coefficients with norms beta^2 - 1, beta^2, beta^2 + 1"""
    logn = 9
    _, pk, _ = frw.synth_triples(logn, 3, seed=5)
    sig, pk, hm, want = FV.bound_triples(logn, pk)
    assert want == [34034725, 34034726, 34034727]
    assert np.count_nonzero(sig) == 6 and np.count_nonzero(FV.v_of(sig, pk, hm)) == 6 and FV.v_of(sig, pk, hm)[:, -1].all()
    for rule in (FV.RULE_CIRCUIT, FV.RULE_SPEC):
        assert FV.norms(sig, pk, hm, rule).tolist() == want
    assert FV.verdicts(want, logn, FV.RULE_CIRCUIT).tolist() == [0, 2, 2]
    assert FV.verdicts(want, logn, FV.RULE_SPEC).tolist() == [0, 0, 2]
    assert [_satisfied(sig[k], pk[k], hm[k], logn) for k in range(3)] == [True, False, False]


def test_a_coefficient_of_6144_is_6145_to_the_circuit():
    logn = 10
    _, pk, _ = frw.synth_triples(logn, 1, seed=6)
    sig, pk, hm, rest = FV.coeff_6144_triple(logn, pk[0])
    beta2 = FV.BETA2[logn]
    assert int(FV.v_of(sig, pk, hm)[0, 5]) == 6144 and rest == beta2 - 6144 ** 2 - 1
    assert FV.norms(sig, pk, hm, FV.RULE_SPEC).tolist() == [beta2 - 1]                  # the specification accepts
    assert FV.norms(sig, pk, hm, FV.RULE_CIRCUIT).tolist() == [beta2 + 12288]           # the circuits do not
    assert not _satisfied(sig[0], pk[0], hm[0], logn)
    # Falcon-512: 6144^2 is over the bound on its own, under either rule
    sig, pk, hm, _ = FV.coeff_6144_triple(9, frw.synth_triples(9, 1, seed=6)[1][0])
    for rule in (FV.RULE_CIRCUIT, FV.RULE_SPEC):
        assert FV.norms(sig, pk, hm, rule)[0] > FV.BETA2[9]
