#!/usr/bin/env python3
"""Time of pht_ctx_estep (include/pht_estep.h) at n = 10, N = 10^6, 64 draws in
one batch, from one run on one box:

* the device time per E-step of its two parts separately (HIP events on the
  context's stream, pht_ctx_estep_ms): the histograms (with the table kernel)
  and the contraction; median of --repeats calls after a warm-up call;
* the uniformisation evaluator (pht_ctx_loglik_unif, totals only) over the
  same draws and observations in the same run, as the yardstick;
* the CPU restatement (tests/estep_spec.c) on one core, timed on a subsample
  of the observations and draws and scaled linearly (the contraction does not
  depend on N: it is timed per draw and not scaled by N).

The draws are bd_exit(n) scaled 0.8 .. 1.25, the observations simulated from
bd_exit(n), --censor of them censored.  Prints one JSON line and writes it to
--out.  Run on the GPU box."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--N", type=int, default=1_000_000)
    ap.add_argument("--draws", type=int, default=64)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--censor", type=float, default=0.3)
    ap.add_argument("--grid-cap", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r11", "estep", "estep_bench.json"))
    a = ap.parse_args()
    if P.device_count() < 1:
        raise SystemExit("estep_bench needs a HIP device: " + P.load().pht_last_error().decode())
    n, N = a.n, a.N
    S, s = bd_exit(n)
    y, cen = simulate_ph(S, s, N, seed=DATA_KEY, censor_frac=a.censor)
    scales = np.linspace(0.8, 1.25, a.draws)
    Ss, ss = [S * c for c in scales], [s * c for c in scales]
    sw = P.Sweeper(n, P.METHODS["ECS"], 1)
    sw.set_obs(y, cen)
    r = sw.estep(Ss, ss, batch=a.batch, grid_cap=a.grid_cap)  # warm-up
    ok = bool(np.all(np.isfinite(r["loglik"])) and np.all(r["nobs"] == N)
              and np.allclose(r["Z"].sum(1), y.sum(), rtol=1e-9))
    hist_ms, con_ms = [], []
    for _ in range(a.repeats):
        sw.estep(Ss, ss, batch=a.batch, grid_cap=a.grid_cap)
        hist_ms.append(float(sw.last_estep_ms[0]))
        con_ms.append(float(sw.last_estep_ms[1]))
    sw.loglik_unif(Ss, ss, batch=a.batch)
    unif_ms = []
    for _ in range(a.repeats):
        u = sw.loglik_unif(Ss, ss, batch=a.batch)
        unif_ms.append(float(sw.last_kernel_ms()))
    ok = ok and all(np.array_equal(u[k], r[k]) for k in ("H", "F", "nbad", "nobs"))
    Ks = [sw.loglik_unif_K(float(np.max(-np.diag(Sk)))) for Sk in Ss]
    sw.close()

    # the restatement on one core: histograms on a subsample, the contraction per draw
    import estep_ref as R

    Nc, Dc = 10_000, 4
    R.spec()
    sub = np.sort(np.random.default_rng(1).choice(N, Nc, replace=False))
    t0 = time.perf_counter()
    hs = [R.hist(Ss[d], ss[d], y[sub], cen[sub], yscale=r["yscale"], ymax=float(y.max())) for d in range(Dc)]
    cpu_hist_s = time.perf_counter() - t0
    win = np.concatenate([h["khi"] - h["klo"] + 1 for h in hs]).astype(np.float64)
    t0 = time.perf_counter()
    for d in range(Dc):
        R.contract(Ss[d], ss[d], r["words"][d], r["yscale"])
    cpu_con_s = time.perf_counter() - t0
    cpu_scaled_s = cpu_hist_s * (N / Nc) * (a.draws / Dc) + cpu_con_s * (a.draws / Dc)

    hmed, cmed, umed = float(np.median(hist_ms)), float(np.median(con_ms)), float(np.median(unif_ms))
    line = {
        "tool": "estep_bench", "n": n, "N": N, "draws": a.draws, "batch": a.batch, "censored": a.censor, "ok": ok,
        "grid_cap": a.grid_cap, "draws_are": "bd_exit(n) scaled 0.8..1.25", "K": [min(Ks), max(Ks)],
        "hist_ms_per_call": {"median": hmed, "min": float(np.min(hist_ms)), "max": float(np.max(hist_ms)),
                             "repeats": len(hist_ms), "all": hist_ms},
        "contract_ms_per_call": {"median": cmed, "min": float(np.min(con_ms)), "max": float(np.max(con_ms)),
                                 "all": con_ms},
        "hist_us_per_draw": 1e3 * hmed / a.draws, "contract_us_per_draw": 1e3 * cmed / a.draws,
        "estep_us_per_draw": 1e3 * (hmed + cmed) / a.draws,
        "loglik_unif_same_run": {"device_ms_per_call_median": umed, "device_us_per_draw": 1e3 * umed / a.draws,
                                 "all": unif_ms},
        "estep_over_loglik_unif": (hmed + cmed) / umed,
        "window": {"mean": float(win.mean()), "max": int(win.max()), "sample": [Dc, Nc]},
        "cpu_restatement_one_core": {"hist_s": cpu_hist_s, "contract_s": cpu_con_s, "at": [Nc, Dc],
                                     "scaled_s": cpu_scaled_s,
                                     "gpu_speedup": cpu_scaled_s / ((hmed + cmed) * 1e-3)},
        "lib_key": P.lib_key(),
    }
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
