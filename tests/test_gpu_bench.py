"""GPU: bench.py's plain run and --dump-outputs.

One small plain run (no --full) in a child process: the line carries the
headline fields and none of the side measurements, and the dumped draws are
the chain this process computes from the same data, priors and seeds (the
dump is reproducible and is what the timed Sweeper.gibbs call returned).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_timed_draws(gpu, tmp_path):
    import phasetype_amd as P
    from phasetype_amd.synth import DATA_KEY, bd_exit, bd_exit_structure, simulate_ph

    n, N, steps, warmup = 5, 3001, 3, 1
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
           str(warmup), "--n", str(n), "--N", str(N), "--dump-outputs", str(out)]
    p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == warmup
    assert line["value"] > 0 and line["unit"] == "iterations/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64"
    assert abs(line["ms_per_step"] * line["value"] - 1e3) < 1e-6 * 1e3
    for side in ("alt_sampler", "weak_scaling", "cpu_baseline", "cpu_best"):
        assert side not in line

    S, s = bd_exit(n)
    T, theta = bd_exit_structure(n)
    nu, zeta = 1.0 + 50.0 * theta, np.full(len(theta), 50.0)
    y, cen = simulate_ph(S, s, N, seed=DATA_KEY)
    sw = P.Sweeper(n, P.METHODS["ECS"], 1, device=0)
    sw.set_obs(y, cen)
    Cm = np.ones(T.shape)
    P.set_seed(20241008)
    warm = sw.gibbs(warmup + 1, P.METHODS["ECS"], nu, zeta, T, Cm, P.zexp_for(y))
    want = sw.gibbs(steps + 1, P.METHODS["ECS"], nu, zeta, T, Cm, P.zexp_for(y), start=warm[-1])
    sw.close()

    assert sorted(os.listdir(out)) == ["draws.npy", "last_draw.npy"]
    draws, last = np.load(out / "draws.npy"), np.load(out / "last_draw.npy")
    assert draws.dtype == np.float64 and draws.shape == (steps + 1, len(theta))
    assert np.array_equal(draws, want)
    assert last.dtype == np.float64 and np.array_equal(last, want[-1])
