#!/usr/bin/env python3
"""Time of pht_ctx_condition (include/pht_condition.h) at n = 10, 10^6 censored
units, 256 draws in batches of 64 and nh = 4 horizons, from one run on one box:

* the device time per call of its two parts separately (HIP events on the
  context's stream, pht_ctx_condition_ms): the table kernels (the (ax, ac)
  table and the forward table F) and the unit kernel, summed over the call's
  batches; median of --repeats calls after a warm-up call, with the range of
  their sum; (draw, unit) pairs per second (draws x units / unit time);
* the wall time of a call beside it: the draws' vectors m and r_h are computed
  on the host inside the call and are in no device time;
* in the same session, on the same context and draws, call by call,
  Sweeper.forecast with the same four horizons (its evaluation time,
  pht_ctx_forecast_ms), the existing per-unit code to compare with, and the
  ratio unit_ms / forecast eval_ms;
* the CPU restatement (tests/condition_spec.c) on a slice of the units and
  draws: its outputs must be the device's bit for bit.

The draws are bd_exit(n) with every rate scattered log-normally (sigma 0.15)
around its value, the ages simulated lifetimes of bd_exit(n), all taken as
still in service, the horizons 0.25, 1, 4 and 16 times the mean age / 8.
Prints one JSON line and writes it to --out.  Run on the GPU box."""
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r15", "condition", "condition_bench.json"))
    a = ap.parse_args()
    if P.device_count() < 1:
        raise SystemExit("condition_bench needs a HIP device: " + P.load().pht_last_error().decode())
    import condition_ref as Cd

    Cd.spec()
    S, s = bd_exit(a.n)
    ages, _ = simulate_ph(S, s, a.units, seed=7)
    cens = np.ones(a.units, np.int32)
    unit = float(np.mean(ages)) / 8.0
    h = unit * np.array([0.25, 1.0, 4.0, 16.0])
    H = len(h)
    Ss, ss = scattered(a.n, a.draws)
    sw = P.Sweeper(a.n, P.METHODS["ECS"], 1)
    sw.set_obs(ages, cens)
    r = sw.condition(Ss, ss, h, batch=a.batch)  # warm-up
    sw.forecast(Ss, ss, h, batch=a.batch)
    tab_ms, unit_ms, wall_ms, fc_tab_ms, fc_ev_ms = [], [], [], [], []
    for _ in range(a.repeats):  # interleaved: both see the same state of the box
        t0 = time.perf_counter()
        sw.condition(Ss, ss, h, batch=a.batch)
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        tab_ms.append(float(sw.last_condition_ms[0]))
        unit_ms.append(float(sw.last_condition_ms[1]))
        sw.forecast(Ss, ss, h, batch=a.batch)
        fc_tab_ms.append(float(sw.last_forecast_ms[0]))
        fc_ev_ms.append(float(sw.last_forecast_ms[1]))
    sw.close()
    # a slice against the restatement (its own context: the same tables need the same largest age)
    cu, cd = min(a.check_units, a.units), min(a.check_draws, a.draws)
    sub = np.argsort(-ages, kind="stable")[:cu]
    sw = P.Sweeper(a.n, P.METHODS["ECS"], 1)
    sw.set_obs(ages[sub], cens[sub])
    g = sw.condition(Ss[:cd], ss[:cd], h, batch=a.batch, pointwise=True)
    sw.close()
    w = Cd.condition(Ss[:cd], ss[:cd], ages[sub], cens[sub], h)
    same = Cd.same_bits(g, w) == []
    ok = bool(same and not r["bad_draw"].any() and not r["nbad"].any())
    um, fe = float(np.median(unit_ms)), float(np.median(fc_ev_ms))
    tot = [x + y for x, y in zip(tab_ms, unit_ms)]
    pairs = a.draws * a.units
    line = {"tool": "condition_bench", "n": a.n, "units": a.units, "draws": a.draws, "batch": a.batch, "nh": H,
            "horizons": h.tolist(), "ok": ok, "bit_equal_to_restatement_on_slice": bool(same),
            "slice": {"units": cu, "draws": cd},
            "draws_are": "bd_exit(n), every rate times exp(0.15 N(0, 1))",
            "device_ms_per_call": {"median": float(np.median(tot)), "min": float(np.min(tot)),
                                   "max": float(np.max(tot)), "repeats": len(tot), "all": tot},
            "table_ms_median": float(np.median(tab_ms)), "table_ms_all": tab_ms,
            "unit_ms_median": um, "unit_ms_all": unit_ms,
            "wall_ms_median": float(np.median(wall_ms)), "wall_ms_all": wall_ms,
            "pairs": pairs, "pairs_per_s": pairs / (um * 1e-3),
            "forecast_eval_ms_median": fe, "forecast_eval_ms_all": fc_ev_ms,
            "forecast_table_ms_median": float(np.median(fc_tab_ms)),
            "unit_over_forecast_eval": um / fe,
            "fleet_mean_residual_life": float(np.mean(r["L"])), "demand_mean": r["Delta"].mean(0).tolist(),
            "demand_sd_between_draws": r["Delta"].std(0).tolist(),
            "phase_mean": r["Phi"].mean(0).tolist(),
            "lib_key": P.lib_key()}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
