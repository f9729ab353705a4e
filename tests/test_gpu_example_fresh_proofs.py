"""examples/pok_fresh_proofs.py as a user runs it: a fresh child process (one seed from the operating system, one device counter, three
seeded proofs and two seeded re-randomisations of the cubic system), which exits 0 only when all five are accepted and share no point."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_example_exits_zero():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "pok_fresh_proofs.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True, timeout=300)
    assert res.returncode == 0, res.stdout
    lines = res.stdout.splitlines()
    assert sum("accepted: True, for y + 1: False" in l for l in lines) == 5, res.stdout
    assert any(l.startswith("no point in common: True; the device counter reads 5") for l in lines), res.stdout
