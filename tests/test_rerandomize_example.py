"""examples/pok_rerandomize.py -- one proof of knowledge of a signature presented three times, on the golden signatures."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_pok_rerandomize_example_runs_on_the_golden_file():
    """The Falcon-512 proofs of examples/pok_prove.py re-randomised twice with factors from `secrets`; examples/pok_verify.py's verifier
    accepts all three sets from (pk, nonce, msg, proof bytes) alone.  The example exits non-zero unless it does and the three sets are
    pairwise different in every one of their three points."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "pok_rerandomize.py"), os.path.join(ROOT, "tests", "golden", "falcon_signed.json"),
                          "--seed", "5"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert sum(l.endswith("verdict [1, 1]") for l in lines) == 3 and lines[-1].startswith("three presentations of 2 statements")
