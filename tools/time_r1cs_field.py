"""Time the satisfaction check over a run-time modulus, frw_r1csf_check_dev, against the hard-wired one in the same process:
Falcon-1024 witnesses over BN254 (4,096 of them = 20.5 GB, or as many as fit; --statements overrides), check only, the caller's
scratch, HIP events around five back-to-back calls after a warm-up -- and frw_r1cs_check_dev on the Montgomery (BLS12-381) witnesses
of the same inputs.  A third figure says what binds: the same call on 32 statements, whose witnesses (160 MB) stay in the 256 MiB
Infinity Cache between calls -- a check that waits on HBM reads gets faster per statement there, one that waits on its own
instructions does not.

Writes both times, their ratio, the witness bytes read per second, the distance to the floor (one read of the witness, 5.0 MB a
statement, at the 6.29 TB/s a copy reaches on this device) and that sentence to --out (default profiles/r1cs_field_check.txt).
usage: python tools/time_r1cs_field.py [--statements K] [--launches 5] [--out PATH]"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import falcon_r1cs_amd as frw

BN254_FR = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
HBM_COPY_RATE = 6.29e12          # bytes/s a float4 copy reaches on an MI355X (8.0 TB/s is the specification)
CACHED_STATEMENTS = 32


def arg(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    import torch
    dev = torch.device("cuda:0")
    eng = frw.WitnessEngine(0)
    launches = arg("--launches", 5)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "r1cs_field_check.txt"), str)
    logn = 10
    L = frw.layout(logn)
    per = (L.num_witness + L.num_instance) * 32
    free_b, _ = torch.cuda.mem_get_info()
    k = arg("--statements", min(4096, int(free_b * 0.85) // (2 * per + 2049 * 32 + 4096)))
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
    # the run-time modulus
    fw, fi = witnesses(eng.field_encoding(BN254_FR))
    hf = eng.r1csf_load(frw.CIRCUIT_NTT, logn, BN254_FR)
    need = eng.r1csf_scratch_bytes(hf, k, False)
    scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    t_field = timed(lambda: eng.r1csf_check_dev(hf, k, fw, fi, num, None, None, scratch, need, s0))
    assert int(num.count_nonzero()) == 0, "a witness over BN254 violates the circuit"
    kc = min(CACHED_STATEMENTS, k)
    t_cached = timed(lambda: eng.r1csf_check_dev(hf, kc, fw, fi, num, None, None, scratch, need, s0))
    eng.r1csf_free(hf)
    del fw, fi, scratch
    # the hard-wired one, on the Montgomery witnesses of the same inputs
    mw, mi = witnesses(frw.ENC_MONTGOMERY)
    hb = eng.r1cs_load(frw.CIRCUIT_NTT, logn)
    t_bls = timed(lambda: eng.r1cs_check_dev(hb, k, mw, mi, num, s0))
    assert int(num.count_nonzero()) == 0
    eng.r1cs_free(hb)
    eng.close()

    read = k * per
    floor = read / HBM_COPY_RATE
    per_stmt, per_stmt_cached = t_field / k, t_cached / kc
    hbm_bound = per_stmt_cached < 0.8 * per_stmt
    binds = ("HBM reads bind: the same check on %d statements whose witnesses stay in the Infinity Cache takes %.1f us a statement against %.1f us from HBM."
             if hbm_bound else
             "Instructions bind, not HBM reads: the same check on %d statements whose witnesses stay in the Infinity Cache takes %.1f us a statement "
             "against %.1f us from HBM, and the witness is read at a fraction of what the memory delivers.") % (kc, per_stmt_cached * 1e6, per_stmt * 1e6)
    lines = [
        "# tools/time_r1cs_field.py: Falcon-1024 NTT circuit, check only, %d statements (%.1f GB of witness and instance), HIP events, mean of %d back-to-back"
        % (k, read / 1e9, launches),
        "# calls after a warm-up, one process",
        "frw_r1csf_check_dev, BN254 Fr (run-time modulus)     %9.3f ms   %7.1f us/statement   %7.1f GB/s of witness read" % (t_field * 1e3, per_stmt * 1e6, read / t_field / 1e9),
        "frw_r1cs_check_dev, BLS12-381 Fr (compiled in)        %9.3f ms   %7.1f us/statement   %7.1f GB/s of witness read" % (t_bls * 1e3, t_bls / k * 1e6, read / t_bls / 1e9),
        "ratio run-time / compiled-in                          %9.2f" % (t_field / t_bls),
        "floor: one read of the witness at %.2f TB/s           %9.3f ms   the run-time check is %.1f x above it" % (HBM_COPY_RATE / 1e12, floor * 1e3, t_field / floor),
        "frw_r1csf_check_dev on %d statements (cache-resident) %9.3f ms   %7.1f us/statement" % (kc, t_cached * 1e3, per_stmt_cached * 1e6),
        binds,
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
