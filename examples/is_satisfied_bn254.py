#!/usr/bin/env python3
"""`assert!(cs.is_satisfied())` (falcon_ntt.rs:159) for a host whose SNARK field is BN254's Fr, on the device.

    python examples/is_satisfied_bn254.py [tests/golden/falcon_signed.json] [--case 0]

A genuine Falcon-512 signature: encoded (public key, message, signature) -> decoders and SHAKE256 on the device -> the witness
over BN254 (frw_ctx_field_encoding, frw_witness_ntt_verify_dev) -> frw_r1csf_check_dev against the circuit's matrices over BN254
(frw_r1csf_load: emitted from the gadget definitions, independently of the witness kernels' closed form).  It says 0 violated rows.
Then one witness element is flipped on the device: the call says how many rows break and which is the first -- ark's
which_is_unsatisfied -- and that row is checked here against the exported matrices (frw_r1cs_export_field), the rows that mention
the flipped variable evaluated with Python integers.

Exit status 0: satisfied, then violated from the row Python says.
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import falcon_r1cs_amd as frw

BN254_FR = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
NONE = 0xFFFFFFFF


def to_ints(a):
    return [int.from_bytes(r.tobytes(), "little") for r in np.ascontiguousarray(a).view(np.uint64).reshape(-1, 4)]


def read_r1cs(path):
    """the FRWR1CS1 file -> (I, W, C, [(row_ptr, col, val)] for A, B, C)"""
    raw = open(path, "rb").read()
    ni, nw, nc, *nnz = np.frombuffer(raw, dtype=np.uint64, count=6, offset=8).tolist()
    off, mats = 56, []
    for k in range(3):
        ptr = np.frombuffer(raw, dtype=np.uint64, count=nc + 1, offset=off); off += 8 * (nc + 1)
        col = np.frombuffer(raw, dtype=np.uint32, count=nnz[k], offset=off); off += 4 * nnz[k]
        val = np.frombuffer(raw, dtype=np.uint64, count=4 * nnz[k], offset=off).reshape(-1, 4); off += 32 * nnz[k]
        mats.append((ptr, col, val))
    return ni, nw, nc, mats


def first_violated_among(mats, rows, z, p):
    for row in rows:
        v = []
        for ptr, col, val in mats:
            lo, hi = int(ptr[row]), int(ptr[row + 1])
            v.append(sum(c * z[int(j)] for c, j in zip(to_ints(val[lo:hi]), col[lo:hi])) % p)
        if (v[0] * v[1] - v[2]) % p:
            return row
    return NONE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("signed", nargs="?", default=os.path.join(ROOT, "tests", "golden", "falcon_signed.json"),
                    help="JSON with cases of {logn, pk_bytes, msg, sig_bytes} (hex)")
    ap.add_argument("--case", type=int, default=0, help="which of the Falcon-512 cases")
    ap.add_argument("--flip", type=int, default=70000, help="the witness element to flip")
    args = ap.parse_args()
    case = [c for c in json.load(open(args.signed))["cases"] if c["logn"] == 9][args.case]
    p, logn = BN254_FR, 9
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    eng = frw.WitnessEngine(0)
    sig, pk, hm, st = eng.prepare_inputs(logn, [bytes.fromhex(case["pk_bytes"])], [bytes.fromhex(case["msg"])], [bytes.fromhex(case["sig_bytes"])])
    if st.any():
        raise SystemExit("the encoded inputs were refused: status %s" % st.tolist())
    L = frw.layout(logn)
    d = [torch.from_numpy(a.view(np.int16)).to(dev) for a in (sig, pk, hm)]
    wit = torch.empty((1, L.num_witness, 4), dtype=torch.int64, device=dev)
    inst = torch.empty((1, L.num_instance, 4), dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    eng.witness_ntt_verify_dev(logn, 1, d[0], d[1], d[2], wit, inst, status, eng.field_encoding(p), stream)

    r1cs = eng.r1csf_load(frw.CIRCUIT_NTT, logn, p)
    info = eng.r1csf_info(r1cs)
    print("the NTT circuit over BN254: I = %d, W = %d, C = %d, %d + %d + %d terms" % (info.num_instance, info.num_witness, info.num_constraints, *info.nnz))
    need = eng.r1csf_scratch_bytes(r1cs, 1, False)
    scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    num = torch.empty(1, dtype=torch.int32, device=dev)
    first = torch.empty(1, dtype=torch.int32, device=dev)
    eng.r1csf_check_dev(r1cs, 1, wit, inst, num, first, None, scratch, need, stream)
    torch.cuda.synchronize()
    satisfied = status.tolist() == [0] and num.tolist() == [0] and first.tolist()[0] & NONE == NONE
    print("the genuine signature: status %d, violated rows: %d" % (status.tolist()[0], num.tolist()[0]))

    wit[0, args.flip, 0] ^= 1
    eng.r1csf_check_dev(r1cs, 1, wit, inst, num, first, None, scratch, need, stream)
    torch.cuda.synchronize()
    got = (num.tolist()[0], first.tolist()[0] & NONE)
    eng.r1csf_free(r1cs)
    eng.close()

    # what Python says: only the rows that mention the flipped variable can have changed
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "ntt9_bn254.r1cs")
        frw.r1cs_export_field(frw.CIRCUIT_NTT, logn, p, path)
        ni, nw, nc, mats = read_r1cs(path)
        mats = [(ptr.copy(), col.copy(), val.copy()) for ptr, col, val in mats]
    column = ni + args.flip
    rows = sorted({int(np.searchsorted(ptr, t, side="right")) - 1 for ptr, col, _ in mats for t in np.flatnonzero(col == column)})
    rinv = pow(1 << 256, -1, p)
    z = [v * rinv % p for v in to_ints(inst[0].cpu().numpy())] + [v * rinv % p for v in to_ints(wit[0].cpu().numpy())]
    want = first_violated_among(mats, rows, z, p)
    print("witness element %d flipped: violated rows: %d, the first is row %d; Python says row %d of the %d rows that read it"
          % (args.flip, got[0], got[1], want, len(rows)))
    if not satisfied or got[0] < 1 or got[1] != want:
        raise SystemExit("expected 0 violated rows for the signature, then at least one from the row Python names")


if __name__ == "__main__":
    main()
