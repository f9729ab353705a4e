#!/usr/bin/env python3
"""The step of the reference's examples/pok_sig.rs that comes before any circuit, on the device:

    assert!(keypair.public_key.verify(msg.as_ref(), &sig));                     pok_sig.rs:21

for a batch of encoded (public key, message, signature) triples: frw_falcon_verify_from_bytes_dev -- both decoders, SHAKE256 and the
verification kernel on one stream, twelve bytes out per signature and no witness.  Verdicts and squared norms under both rules:
FRW_RULE_CIRCUIT (accepted = the signature can be proven by the three circuits) and FRW_RULE_SPEC (the Falcon specification's Verify).
Then the same triples with one message byte flipped (a byte appended to an empty message).

    python examples/falcon_verify.py tests/golden/falcon_signed.json

Exit status 0: every genuine triple was accepted under both rules and every tampered one refused.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import falcon_r1cs_amd as frw

STATUS = {frw.ST_OK: "accepted", frw.ST_COEFF_RANGE: "refused (coefficient range)", frw.ST_NORM_BOUND: "refused (norm bound)",
          frw.ST_DECODE: "refused (malformed encoding)"}
RULES = ((frw.RULE_CIRCUIT, "circuit"), (frw.RULE_SPEC, "spec"))


def flipped(msg):
    return bytes([msg[0] ^ 1]) + msg[1:] if msg else b"\x01"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("signed", help="JSON with cases of {logn, pk_bytes, msg, sig_bytes} (hex)")
    args = ap.parse_args()
    cases = json.load(open(args.signed))["cases"]
    eng = frw.WitnessEngine(0)
    ok = True
    for logn in (9, 10):
        sel = [c for c in cases if c["logn"] == logn]
        if not sel:
            continue
        pkb, msgs, sgb = ([bytes.fromhex(c[k]) for c in sel] for k in ("pk_bytes", "msg", "sig_bytes"))
        for title, batch_msgs, want_accepted in (("genuine", msgs, True), ("one message byte flipped", [flipped(m) for m in msgs], False)):
            print("Falcon-%d, %d signatures, %s" % (1 << logn, len(sel), title))
            for rule, name in RULES:
                d_status, d_norm = eng.falcon_verify_from_bytes_dev(logn, pkb, sgb, batch_msgs, rule)
                torch.cuda.synchronize()
                for k, (st, norm) in enumerate(zip(d_status.tolist(), d_norm.tolist())):
                    print("  %-7s rule, signature %d: %s, squared norm %s" % (name, k, STATUS[st], norm if norm >= 0 else "-"))
                    ok &= (st == frw.ST_OK) == want_accepted
    eng.close()
    if not ok:
        raise SystemExit("expected every genuine signature accepted and every tampered one refused")


if __name__ == "__main__":
    main()
