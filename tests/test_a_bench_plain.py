"""A plain `bench.py` run does only what its headline needs (set up, warm up, time the steps, check the statuses, dump the
outputs if asked, print the line); everything else it measures or checks runs with --full.  Both in child processes, so
this file, like the multi-rank one, runs before the -m gpu suite's own process has touched the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline"}


def _run(args, timeout=600):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "bench.py"] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_a_plain_run_prints_the_headline_alone_and_full_adds_the_rest(tmp_path):
    small = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "512", "--chunk", "256"]
    plain = _run(small + ["--dump-outputs", str(tmp_path / "plain")])
    assert set(plain) == HEADLINE, sorted(plain)
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["config"]["signatures_failing_range_checks"] == 0
    assert plain["roofline"]["launches_timed"] == 4 and "device_write_stream_GBs" not in plain["roofline"]
    full = _run(small + ["--full", "--no-secondary", "--dump-outputs", str(tmp_path / "full")])
    assert set(full) == HEADLINE | {"launch_shape_checked", "r1cs_check", "cpu_baseline"}, sorted(full)
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "n_gpus"):
        assert plain[k] == full[k], k
    assert full["r1cs_check"]["witnesses_checked"] == 256 and full["r1cs_check"]["unsatisfied"] == 0
    assert full["launch_shape_checked"]["distinct_digests"] == 256
    assert full["cpu_baseline"]["gpu_witnesses_checked_by_digest"] == 256
    assert full["roofline"]["device_write_stream_GBs"] > 0
    # the same timed steps: what the last one left is the same with and without --full
    names = sorted(os.listdir(str(tmp_path / "plain")))
    assert names == sorted(os.listdir(str(tmp_path / "full"))) and len(names) == 5
    for name in names:
        assert np.array_equal(np.load(str(tmp_path / "plain" / name)), np.load(str(tmp_path / "full" / name))), name


def test_the_plan_of_a_plain_run_holds_no_legs():
    """--plan describes the run its arguments describe: the gather and proof legs of an N > 1 run, and the sharded aggregate proof,
    belong to --full runs only."""
    def plan(*extra):
        out = subprocess.run([sys.executable, "bench.py", "--plan"] + list(extra), cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    plain, full = plan(), plan("--full")
    for world in (1, 2, 4, 8):
        p, f = plain["gpus_%d" % world], full["gpus_%d" % world]
        assert p["global_index_range_per_rank"] == f["global_index_range_per_rank"] and p["chunk"] == f["chunk"]
        assert p["fits"] and f["fits"] and p["hbm_plan_bytes_per_rank"] <= f["hbm_plan_bytes_per_rank"]
        assert not any(k.startswith("aggregate_proof_sharded") for k in p)
        assert any(k.startswith("aggregate_proof_sharded") for k in f)
        assert not p["gather"]
        assert bool(f["gather"]) == (world > 1)
