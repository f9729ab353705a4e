"""Golden digests of the schoolbook circuit's witness for two fixture triples per parameter set.

Everything comes from the ORACLE side: oracle/falcon_gadgets.py::FalconSchoolBookVerificationCircuit run on
oracle/ark_sim.py, checked with is_satisfied() before anything is written.  Each file holds the inputs as hex, the counts,
how many columns take each of the two tails, and the sha256 of the witness and instance bytes in both encodings -- digests
only, no witness bytes (a Falcon-1024 witness is 36.8 MB).  The product is not involved.
    python tests/golden/make_schoolbook.py     (about two minutes)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import schoolbook_ref as S  # noqa: E402


def main():
    for logn in (9, 10):
        n = 1 << logn
        out = {"logn": logn, "triples": []}
        for which, seed in enumerate(S.SEEDS[logn]):
            sig, pk, hm = S.triple(logn, seed)
            cs = S.oracle_cs(sig, pk, hm, logn, strict=True)
            assert cs.is_satisfied()
            i, w, c = S.counts(logn)
            assert (cs.num_instance_variables(), cs.num_witness_variables(), cs.num_constraints()) == (i, w, c)
            out["counts"] = {"num_instance": i, "num_witness": w, "num_constraints": c}
            lt, ge = S.tail_counts(cs, logn)
            assert lt + ge == n and 10 * lt >= n and 10 * ge >= n, (lt, ge)
            digests = {}
            for name, mont in (("canonical", False), ("montgomery", True)):
                wit, inst = S.encoded(cs, mont)
                digests[name] = {"witness": S.sha(wit), "instance": S.sha(inst)}
            out["triples"].append({"seed": seed, "sig": sig.tobytes().hex(), "pk": pk.tobytes().hex(), "hm": hm.tobytes().hex(),
                                   "tails": {"hm_lt_c": lt, "hm_ge_c": ge}, "sha256": digests})
            print(logn, seed, lt, ge, flush=True)
        with open(os.path.join(HERE, "schoolbook_%d.json" % n), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
