"""GPU: bench.py's command line.  A plain run prints the headline line alone;
--full adds the per-kernel / roofline objects of the same timed steps;
--dump-outputs writes the error counters of the last timed step, the same from
run to run and equal to a direct dsce_run over that step's realisations."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import harness

pytestmark = pytest.mark.gpu

STEPS, WARMUP, B = 3, 1, 1024          # 1024 realisations per step: 16 waves, more than one block
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY = {"roofline", "kernels", "step_roofline", "work_per_scheme", "cpu_baseline"}


def _bench(*extra):
    out = subprocess.run([sys.executable, os.path.join(harness.ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                          "--warmup", str(WARMUP), "--reps-per-step", str(B), *extra],
                         check=True, timeout=120, capture_output=True, text=True)
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench")
    plain = _bench("--dump-outputs", str(d / "a"))
    full = _bench("--full", "--no-cpu-baseline", "--dump-outputs", str(d / "b"))
    return plain, full, d


def test_plain_line_is_the_headline_and_full_adds_the_rest(runs):
    plain, full, _ = runs
    for line in (plain, full):
        assert HEADLINE <= set(line)
        assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["dtype"] == "f64"
        assert line["unit"] == "realisations/s" and line["higher_is_better"] is True
        # value and ms_per_step describe the same timed steps
        assert line["value"] == pytest.approx(B * 1e3 / line["ms_per_step"], rel=1e-9)
    assert plain["full"] is False and not FULL_ONLY & set(plain)
    assert full["full"] is True and FULL_ONLY <= set(full)
    assert full["cpu_baseline"] is None                   # --no-cpu-baseline
    assert full["roofline"]["peak_measured"] > 0 and full["kernels"]
    assert plain["metric"] == full["metric"] == bench.METRIC


def test_dumped_outputs_are_the_last_steps_counters(runs):
    _, _, d = runs
    a, b = np.load(d / "a" / "err_counts.npy"), np.load(d / "b" / "err_counts.npy")
    assert a.dtype == np.float64 and sorted(os.listdir(d / "a")) == ["err_counts.npy"]
    assert np.array_equal(a, b)                           # equal arguments, equal inputs, equal counters
    from dsce.configs import build_setup
    from dsce.engine import build_engine, gpu_tx
    name, schemes, _, _ = bench.WORKLOADS["c2"]
    eng = build_engine(build_setup(name, schemes=schemes, tx=gpu_tx(0)), batch=B)
    try:
        ref = eng.run(bench.SEED, (WARMUP + STEPS - 1) * B, B)
    finally:
        eng.close()
    assert a.shape == ref.shape and ref.sum() > 0
    assert np.array_equal(a, ref.astype(np.float64))
