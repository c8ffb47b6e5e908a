#!/usr/bin/env python3
"""Time of a PSIS-LOO (Sweeper.psis_loo's steps) at n = 10, N = 10^6 with 256
and 1,024 draws in batches of 64: the fill of the device matrix
(pht_ctx_loo_fill: the spectral log-likelihood kernel in pointwise mode,
its rows kept on the device) and the PSIS pass (pht_ctx_loo: the chunked
transpose and one wavefront per observation), separately.

Both are device times of the call's kernel launches (HIP events on the
context's stream, pht_ctx_last_kernel_ms), median of --repeats calls after a
warm-up, with the range.  Next to them the CPU restatement of
include/pht_psis.h (tests/psis_spec.c) on one core, timed on a slice of the
GPU's own matrix columns and scaled linearly in the observations.  Prints one
JSON line per draw count and writes them to --out.  Run on the GPU box."""
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
from phasetype_amd.synth import DATA_KEY, bd_exit, simulate_ph  # noqa: E402


def _stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms)), "repeats": len(ms),
            "all": [float(v) for v in ms]}


def draws_around(S0, s0, nd, seed=1):
    """nd generators around (S0, s0): every rate scaled by c_d, the exit
    rates by e_d as well"""
    rng = np.random.default_rng(seed)
    c, e = np.exp(rng.normal(0.0, 0.05, nd)), np.exp(rng.normal(0.0, 0.1, nd))
    off = S0 - np.diag(np.diag(S0))
    Ss, ss = [], []
    for cd, ed in zip(c, e):
        s = s0 * cd * ed
        A = off * cd
        Ss.append(A - np.diag(A.sum(axis=1) + s))
        ss.append(s)
    return Ss, ss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--N", type=int, default=1_000_000)
    ap.add_argument("--draws", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cpu-obs", type=int, default=200, help="observations of the restatement's slice")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r10", "loo", "loo_bench.json"))
    a = ap.parse_args()
    if P.device_count() < 1:
        raise SystemExit("loo_bench needs a HIP device: " + P.load().pht_last_error().decode())
    import psis_ref as R

    n, N = a.n, a.N
    S, s = bd_exit(n)
    y, cen = simulate_ph(S, s, N, seed=DATA_KEY, censor_frac=0.1)
    Ss, ss = draws_around(S, s, max(a.draws))
    blocks = np.stack([P.loglik_block(A, b) for A, b in zip(Ss, ss)])
    sw = P.Sweeper(n, P.METHODS["ECS"], 1)
    sw.set_obs(y, cen)
    lines = []
    for nd in a.draws:
        b = blocks[:nd]
        sw.loo_begin(nd)
        fill_ms, psis_ms = [], []
        for k in range(a.repeats + 1):  # the first is the warm-up
            sw.loo_fill(0, blocks=b, batch=a.batch)
            f = float(sw.last_kernel_ms())
            r = sw.loo_result()
            if k:
                fill_ms.append(f)
                psis_ms.append(float(sw.last_kernel_ms()))
        sw.loo_end()
        ok = bool(np.all(r["flags"] == 0) and np.all(np.isfinite(r["elpd_i"])))
        # the restatement on one core, on the GPU's own values of a slice
        Nc = min(a.cpu_obs, N)
        pick = np.linspace(0, N - 1, Nc).astype(np.int64)
        sub = P.Sweeper(n, P.METHODS["ECS"], 1)
        sub.set_obs(y[pick], cen[pick])
        l = sub.loglik_blocks(b, pointwise=True)["pointwise"]
        sub.close()
        R.spec()
        t0 = time.perf_counter()
        want = R.psis(l)
        cpu_s = time.perf_counter() - t0
        same = all(np.array_equal(r[k][pick].view(np.uint64), want[k].view(np.uint64))
                   for k in ("elpd_i", "khat", "lppd_i"))
        fm, pm = float(np.median(fill_ms)), float(np.median(psis_ms))
        khat = r["khat"]
        line = {
            "tool": "loo_bench", "n": n, "N": N, "draws": nd, "batch": a.batch, "ok": ok,
            "slice_bit_identical_to_restatement": bool(same),
            "fill_device_ms": _stats(fill_ms), "psis_device_ms": _stats(psis_ms),
            "psis_over_fill": pm / fm, "psis_us_per_observation": 1e3 * pm / N,
            "matrix_GB": 8.0 * nd * N / 1e9, "tail_length": R.tail_len(nd),
            "khat": {"median": float(np.median(khat)), "max": float(np.max(khat)),
                     "above_0.7": int(np.sum(khat > 0.7))},
            "elpd_loo": float(np.sum(r["elpd_i"])), "p_loo": float(np.sum(r["p_loo_i"])),
            "cpu_restatement_one_core": {"measured_s": cpu_s, "observations": Nc, "scaled_s": cpu_s * N / Nc,
                                         "gpu_speedup_psis": cpu_s * N / Nc / (pm * 1e-3)},
            "lib_key": P.lib_key(),
        }
        print(json.dumps(line), flush=True)
        lines.append(line)
    sw.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
