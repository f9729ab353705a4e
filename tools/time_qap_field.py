"""Time the QAP witness map over a run-time modulus, frw_qapf_witness_map_dev, against the hard-wired one in the same process: 256
Falcon-1024 NTT statements (domain 2^18; --statements overrides), HIP events around five back-to-back calls after a warm-up --
  frw_qapf_witness_map_dev over BN254's Fr (generator 5),
  frw_qapf_witness_map_dev over BLS12-381's r (generator 7),
  frw_qap_witness_map_dev over r on the same inputs: the code with the modulus compiled in, the yardstick
-- and next to the times the field products the map needs, 7 (n / 2) log2 n in the butterflies + about 5 n per-index factors and the
a o b products a statement, against what the multiplier issues (frw_diag_valu_rates: a product over a run-time modulus is eight CIOS rounds
of sixteen v_mad_u64_u32).  A record, judged against nothing.

Writes the figures to --out (default profiles/qap_field_map.txt).
usage: python tools/time_qap_field.py [--statements K] [--launches 5] [--out PATH]"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import falcon_r1cs_amd as frw

BN254_FR = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
BLS12_381_FR = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
FIELD_MUL_MAD64 = 8 * 16         # v_mad_u64_u32 of one field_mul: eight rounds of x K and m p over eight limbs


def arg(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    import torch
    dev = torch.device("cuda:0")
    eng = frw.WitnessEngine(0)
    launches = arg("--launches", 5)
    k = arg("--statements", 256)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "qap_field_map.txt"), str)
    logn = 10
    L = frw.layout(logn)
    s0 = torch.cuda.current_stream().cuda_stream
    sig, pk, hm = frw.synth_triples(logn, min(k, 64), seed=5)
    rep = (k + sig.shape[0] - 1) // sig.shape[0]
    d = [torch.from_numpy(np.tile(a, (rep, 1))[:k].copy().view(np.int16)).to(dev) for a in (sig, pk, hm)]

    def witnesses(enc):
        wit = torch.empty((k, L.num_witness, 4), dtype=torch.int64, device=dev)
        inst = torch.empty((k, L.num_instance, 4), dtype=torch.int64, device=dev)
        st = torch.empty(k, dtype=torch.int32, device=dev)
        eng.witness_ntt_verify_dev(logn, k, d[0], d[1], d[2], wit, inst, st, enc, s0)
        torch.cuda.synchronize()
        assert int((st != 0).sum()) == 0
        return wit, inst

    def timed(fn):
        fn()                                                     # warm-up
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / launches / 1e3

    num = torch.empty(k, dtype=torch.int32, device=dev)

    def field_map(p, g, wit, inst):
        """-> (seconds a call, h, log n, passes)"""
        hf = eng.r1csf_load(frw.CIRCUIT_NTT, logn, p)
        q = eng.qapf_create(hf, g)
        info = eng.qapf_info(q)
        n, per = int(info.domain.size), int(info.workspace_bytes_per_statement)
        ws = torch.empty(k * per, dtype=torch.uint8, device=dev)
        h = torch.empty((k, n, 4), dtype=torch.int64, device=dev)
        t = timed(lambda: eng.qapf_witness_map_dev(q, k, wit, inst, h, ws, k * per, num, s0))
        assert int(num.count_nonzero()) == 0, "a witness violates the circuit"
        eng.qapf_free(q)
        eng.r1csf_free(hf)
        return t, h, int(info.domain.log_size), int(info.num_passes)

    fw, fi = witnesses(eng.field_encoding(BN254_FR))
    t_bn, h_bn, log_n, passes = field_map(BN254_FR, 5, fw, fi)
    del fw, fi, h_bn
    mw, mi = witnesses(frw.ENC_MONTGOMERY)
    t_r, h_r, _, _ = field_map(BLS12_381_FR, 7, mw, mi)
    hb = eng.r1cs_load(frw.CIRCUIT_NTT, logn)
    qi = eng.qap_info(hb)
    per = int(qi.workspace_bytes_per_signature)
    ws = torch.empty(k * per, dtype=torch.uint8, device=dev)
    h_hard = torch.empty_like(h_r)
    t_hard = timed(lambda: eng.qap_witness_map_dev(hb, k, mw, mi, h_hard, ws, k * per, num, s0))
    assert int(num.count_nonzero()) == 0
    assert torch.equal(h_r, h_hard), "over r the two maps differ"
    eng.r1cs_free(hb)
    rates = eng.valu_rates()
    eng.close()

    n = 1 << log_n
    products = 7 * (n // 2) * log_n + 5 * n
    achieved = products * k / t_bn
    peak = rates["simds"] * 64 * rates["v_mad_u64_u32"] * 1e6 / FIELD_MUL_MAD64
    lines = [
        "# tools/time_qap_field.py: Falcon-1024 NTT circuit, %d statements, domain 2^%d, %d passes a transform; HIP events, mean of %d back-to-back"
        % (k, log_n, passes, launches),
        "# calls after a warm-up, one process; over r the two maps' h are byte-equal",
        "frw_qapf_witness_map_dev, BN254 Fr, g = 5 (run-time modulus)      %9.3f ms   %8.1f us/statement" % (t_bn * 1e3, t_bn / k * 1e6),
        "frw_qapf_witness_map_dev, BLS12-381 Fr, g = 7 (run-time modulus)  %9.3f ms   %8.1f us/statement" % (t_r * 1e3, t_r / k * 1e6),
        "frw_qap_witness_map_dev, BLS12-381 Fr (compiled in)               %9.3f ms   %8.1f us/statement" % (t_hard * 1e3, t_hard / k * 1e6),
        "ratio run-time / compiled-in over r                               %9.2f" % (t_r / t_hard),
        "ratio BN254 run-time / compiled-in                                %9.2f" % (t_bn / t_hard),
        "field products a statement: 7 (n / 2) log2 n + 5 n                %9.3f M" % (products / 1e6),
        "achieved over BN254 (the check's products not counted)            %9.1f G products/s" % (achieved / 1e9),
        "the multiplier's bound: %d SIMDs x 64 lanes x %.1f v_mad_u64_u32 wave-instructions/SIMD/us / %d a product   %9.1f G products/s (%.0f %% reached)"
        % (rates["simds"], rates["v_mad_u64_u32"], FIELD_MUL_MAD64, peak / 1e9, 100 * achieved / peak),
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
