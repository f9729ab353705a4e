"""examples/pok_prove.py -- the prover's side of the reference's examples/pok_sig.rs as one call, on the golden signatures."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_pok_prove_example_runs_on_the_golden_file():
    """All Falcon-512 cases of tests/golden/falcon_signed.json and a tampered copy of the first through ONE call of
    frw_pok_prove_from_bytes_dev; the verifier's side accepts every proof from (pk, nonce, msg, proof bytes) alone.  The example exits
    non-zero unless every genuine case is proven and accepted and the tampered one is refused with all-zero proof bytes."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "pok_prove.py"), os.path.join(ROOT, "tests", "golden", "falcon_signed.json"),
                          "--seed", "5"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("  case ")]
    assert len(lines) == 3 and sum("(tampered)" in l for l in lines) == 1
    for l in lines:
        if "(tampered)" in l:
            assert "prover status 0" not in l and "proof 0000000000000000..." in l and "verdict 1" not in l
        else:
            assert "prover status 0" in l and l.endswith("statement 0, verdict 1")
