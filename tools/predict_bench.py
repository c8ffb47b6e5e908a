#!/usr/bin/env python3
"""Time of pht_ctx_predict (totals mode: words, extremes, histogram; the
production path of ``ppc``) at n = 10: 256 BD-exit(10) draws scaled 0.8 .. 1.25
in batches of 64, 10^6 replicates each, 64 edges.

The time is the device time of the call's kernel launches (HIP events on the
context's stream, pht_ctx_last_kernel_ms), median of --repeats calls after a
warm-up call, with the range.  paths/s = draws x replicates over that time;
jumps/s from the ``njump`` words of the call (every jump is one exponential
sojourn, one categorical draw and their Philox words).  Next to it the CPU
restatement of include/pht_predict.h (tests/predict_spec.c) on one core, timed
on a scaled-down share of the same work (--cpu-draws x --cpu-reps) and scaled
linearly.  Prints one JSON line and writes it to --out.  Run on the GPU box."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import phasetype_amd as P  # noqa: E402
from phasetype_amd.synth import bd_exit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--reps", type=int, default=1_000_000)
    ap.add_argument("--draws", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--edges", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cpu-draws", type=int, default=4)
    ap.add_argument("--cpu-reps", type=int, default=50_000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r09", "predict", "predict_bench.json"))
    a = ap.parse_args()
    if P.device_count() < 1:
        raise SystemExit("predict_bench needs a HIP device: " + P.load().pht_last_error().decode())
    import predict_ref as R

    S, s = bd_exit(a.n)
    scales = np.linspace(0.8, 1.25, a.draws)
    Ss, ss = [S * c for c in scales], [s * c for c in scales]
    m1 = R.moments(S)[0]
    edges = np.linspace(0.05, 4.0, a.edges) * m1
    key = R.KEY

    sw = P.Sweeper(a.n, P.METHODS["ECS"], 1)
    call = lambda: sw.predict(Ss, ss, a.reps, key=key, edges=edges, batch=a.batch)  # noqa: E731
    r = call()  # warm-up
    dev_ms, wall_ms = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        call()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(float(sw.last_kernel_ms()))
    sw.close()
    paths, jumps = int(r["ndone"].sum() + r["nbad"].sum()), int(r["njump"].sum())
    mid = a.draws // 2
    ok = bool(np.all(r["nbad"] == 0) and np.all(r["ndone"] == a.reps) and paths == a.draws * a.reps
              and abs(r["mean"][mid] * scales[mid] / m1 - 1.0) < 0.01)

    # the restatement on one core, a share of the same work
    R.spec()
    pick = np.linspace(0, a.draws - 1, a.cpu_draws).astype(int)
    t0 = time.perf_counter()
    rc = R.predict([Ss[k] for k in pick], [ss[k] for k in pick], a.cpu_reps, edges=edges)
    cpu_s = time.perf_counter() - t0
    cpu_jumps = int(rc["njump"].sum())
    cpu_scaled_s = cpu_s * jumps / cpu_jumps

    med = float(np.median(dev_ms))
    line = {
        "tool": "predict_bench", "n": a.n, "draws": a.draws, "reps": a.reps, "batch": a.batch, "edges": a.edges,
        "mode": "totals", "ok": ok, "draws_are": "bd_exit(n) scaled 0.8..1.25",
        "device_ms_per_call": {"median": med, "min": float(np.min(dev_ms)), "max": float(np.max(dev_ms)),
                               "repeats": len(dev_ms), "all": dev_ms},
        "wall_ms_per_call_median": float(np.median(wall_ms)),
        "paths": paths, "jumps": jumps, "jumps_per_path": jumps / paths,
        "paths_per_s": paths / (med * 1e-3), "jumps_per_s": jumps / (med * 1e-3),
        "cpu_restatement_one_core": {"measured_s": cpu_s, "at": [int(a.cpu_draws), int(a.cpu_reps)],
                                     "jumps": cpu_jumps, "jumps_per_s": cpu_jumps / cpu_s, "scaled_s": cpu_scaled_s,
                                     "gpu_speedup": cpu_scaled_s / (med * 1e-3)},
        "lib_key": P.lib_key(),
    }
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
