#!/usr/bin/env python3
"""Time of pht_ctx_forecast (include/pht_forecast.h) at n = 10, 10^6 censored
units, 256 draws in batches of 64 and H = 4 horizons, from one run on one box:

* the device time per call of its two parts separately (HIP events on the
  context's stream, pht_ctx_forecast_ms): the table kernel and the
  evaluations, summed over the call's batches; median of --repeats calls after
  a warm-up call, with the range of their sum; evaluations of the survival
  function per second (draws x units x (H + 1) / eval time);
* in the same session, on the same context and draws, Sweeper.loglik_unif
  (totals only; device time, pht_ctx_last_kernel_ms, tables included), the
  existing code to compare with, and the ratio
  eval_ms / ((H + 1) loglik_unif_ms): above 1, the H + 1 evaluations per unit
  cost more than H + 1 separate likelihood passes would;
* the CPU restatement (tests/forecast_spec.c) on a slice of the units and
  draws: its words must be the device's bit for bit.

The draws are bd_exit(n) with every rate scattered log-normally (sigma 0.15)
around its value, the ages simulated lifetimes of bd_exit(n), all taken as
still in service, the horizons 0.25, 1, 4 and 16 times the mean age / 8.
Prints one JSON line and writes it to --out.  Run on the GPU box."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import phasetype_amd as P  # noqa: E402
from phasetype_amd.synth import bd_exit, simulate_ph  # noqa: E402
from quantile_bench import scattered  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--units", type=int, default=1000000)
    ap.add_argument("--draws", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--check-units", type=int, default=2000)
    ap.add_argument("--check-draws", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r13", "forecast", "forecast_bench.json"))
    a = ap.parse_args()
    if P.device_count() < 1:
        raise SystemExit("forecast_bench needs a HIP device: " + P.load().pht_last_error().decode())
    import forecast_ref as F

    F.spec()
    S, s = bd_exit(a.n)
    ages, _ = simulate_ph(S, s, a.units, seed=7)
    cens = np.ones(a.units, np.int32)
    unit = float(np.mean(ages)) / 8.0
    h = unit * np.array([0.25, 1.0, 4.0, 16.0])
    H = len(h)
    Ss, ss = scattered(a.n, a.draws)
    sw = P.Sweeper(a.n, P.METHODS["ECS"], 1)
    sw.set_obs(ages, cens)
    r = sw.forecast(Ss, ss, h, batch=a.batch)  # warm-up
    tab_ms, ev_ms, ll_ms = [], [], []
    for _ in range(a.repeats):  # interleaved: both see the same state of the box
        sw.forecast(Ss, ss, h, batch=a.batch)
        tab_ms.append(float(sw.last_forecast_ms[0]))
        ev_ms.append(float(sw.last_forecast_ms[1]))
        sw.loglik_unif(Ss, ss, batch=a.batch)
        ll_ms.append(float(sw.last_kernel_ms()))
    sw.close()
    # a slice against the restatement (its own context: the same tables need the same largest age)
    cu, cd = min(a.check_units, a.units), min(a.check_draws, a.draws)
    sub = np.argsort(-ages, kind="stable")[:cu]
    sw = P.Sweeper(a.n, P.METHODS["ECS"], 1)
    sw.set_obs(ages[sub], cens[sub])
    g = sw.forecast(Ss[:cd], ss[:cd], h, batch=a.batch, pointwise=True)
    sw.close()
    w = F.forecast(Ss[:cd], ss[:cd], ages[sub], cens[sub], h)
    same = F.same_bits(g, w) == []
    ok = bool(same and not r["bad_draw"].any() and not r["nbad"].any())
    ev, ll = float(np.median(ev_ms)), float(np.median(ll_ms))
    tot = [x + y for x, y in zip(tab_ms, ev_ms)]
    evals = a.draws * a.units * (H + 1)
    mom = P.forecast_moments(r["M"], r["V"])
    line = {"tool": "forecast_bench", "n": a.n, "units": a.units, "draws": a.draws, "batch": a.batch, "H": H,
            "horizons": h.tolist(), "ok": ok, "bit_equal_to_restatement_on_slice": bool(same),
            "slice": {"units": cu, "draws": cd},
            "draws_are": "bd_exit(n), every rate times exp(0.15 N(0, 1))",
            "device_ms_per_call": {"median": float(np.median(tot)), "min": float(np.min(tot)),
                                   "max": float(np.max(tot)), "repeats": len(tot), "all": tot},
            "table_ms_median": float(np.median(tab_ms)), "eval_ms_median": ev, "eval_ms_all": ev_ms,
            "evaluations": evals, "evaluations_per_s": evals / (ev * 1e-3),
            "loglik_unif_ms_median": ll, "loglik_unif_ms_all": ll_ms,
            "eval_over_H_plus_1_loglik_unif": ev / ((H + 1) * ll),
            "expected_failures": mom["mean"].tolist(), "sd": mom["sd"].tolist(),
            "lib_key": P.lib_key()}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
