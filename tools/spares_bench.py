#!/usr/bin/env python3
"""Time of pht_ctx_spares (include/pht_spares.h) at n = 10, 10^6 censored units,
256 draws in batches of 64 and nh = 4 horizons, from one run on one box:

* the device time per call of its two parts separately (HIP events on the
  context's stream, pht_ctx_spares_ms): the vectors kernel with the table
  kernels (the (ax, ac) table and the forward table F), and the unit kernel,
  summed over the call's batches; median of --repeats calls after a warm-up
  call, with the range of their sum; (draw, unit) pairs per second (draws x
  units / unit time); the wall time of a call beside it;
* in the same session, on the same context, draws and horizons, call by call,
  Sweeper.condition (pht_ctx_condition_ms and its wall time): it computes the
  mean D alone and builds the draws' vectors on the host inside the call, which
  is in its wall time and in no device time;
* a second pair of calls at a long horizon (mu h_max about 1000, Kr about
  1500), where the vectors cost the most: the vectors time of spares beside
  the wall time of condition;
* the CPU restatement (tests/spares_spec.c) on a slice of the units and draws:
  its outputs must be the device's bit for bit.

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


def _pair(sw, Ss, ss, h, batch, repeats):
    """spares and condition interleaved call by call: both see the same state of the box"""
    out = {k: [] for k in ("vec_ms", "unit_ms", "wall_ms", "cd_tab_ms", "cd_unit_ms", "cd_wall_ms")}
    for _ in range(repeats):
        t0 = time.perf_counter()
        sw.spares(Ss, ss, h, batch=batch)
        out["wall_ms"].append((time.perf_counter() - t0) * 1e3)
        out["vec_ms"].append(float(sw.last_spares_ms[0]))
        out["unit_ms"].append(float(sw.last_spares_ms[1]))
        t0 = time.perf_counter()
        sw.condition(Ss, ss, h, batch=batch)
        out["cd_wall_ms"].append((time.perf_counter() - t0) * 1e3)
        out["cd_tab_ms"].append(float(sw.last_condition_ms[0]))
        out["cd_unit_ms"].append(float(sw.last_condition_ms[1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--units", type=int, default=1000000)
    ap.add_argument("--draws", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--long-repeats", type=int, default=3)
    ap.add_argument("--check-units", type=int, default=2000)
    ap.add_argument("--check-draws", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r18", "spares", "spares_bench.json"))
    a = ap.parse_args()
    if P.device_count() < 1:
        raise SystemExit("spares_bench needs a HIP device: " + P.load().pht_last_error().decode())
    import spares_ref as Sp

    Sp.spec()
    S, s = bd_exit(a.n)
    ages, _ = simulate_ph(S, s, a.units, seed=7)
    cens = np.ones(a.units, np.int32)
    unit = float(np.mean(ages)) / 8.0
    h = unit * np.array([0.25, 1.0, 4.0, 16.0])
    H = len(h)
    Ss, ss = scattered(a.n, a.draws)
    mu_max = max(float(np.max(-np.diag(A))) for A in Ss)
    h_long = h * (1000.0 / (mu_max * h[-1]))
    sw = P.Sweeper(a.n, P.METHODS["ECS"], 1)
    sw.set_obs(ages, cens)
    r = sw.spares(Ss, ss, h, batch=a.batch)  # warm-up
    c = sw.condition(Ss, ss, h, batch=a.batch)
    t = _pair(sw, Ss, ss, h, a.batch, a.repeats)
    rl = sw.spares(Ss, ss, h_long, batch=a.batch)
    tl = _pair(sw, Ss, ss, h_long, a.batch, a.long_repeats)
    sw.close()
    # a slice against the restatement (its own context: the same tables need the same largest age)
    cu, cd = min(a.check_units, a.units), min(a.check_draws, a.draws)
    sub = np.argsort(-ages, kind="stable")[:cu]
    sw = P.Sweeper(a.n, P.METHODS["ECS"], 1)
    sw.set_obs(ages[sub], cens[sub])
    g = sw.spares(Ss[:cd], ss[:cd], h, batch=a.batch, pointwise=True)
    sw.close()
    w = Sp.spares(Ss[:cd], ss[:cd], ages[sub], cens[sub], h)
    same = Sp.same_bits(g, w) == []
    same_d = bool(np.array_equal(r["Delta"], c["Delta"]) and np.array_equal(r["dsum"], c["dsum"]))
    ok = bool(same and same_d and not r["bad_draw"].any() and not r["nbad"].any())
    med = {k: float(np.median(v)) for k, v in t.items()}
    medl = {k: float(np.median(v)) for k, v in tl.items()}
    tot = [x + y for x, y in zip(t["vec_ms"], t["unit_ms"])]
    cd_tot = [x + y for x, y in zip(t["cd_tab_ms"], t["cd_unit_ms"])]
    pairs = a.draws * a.units
    mom = P.forecast_moments(r["Delta"], r["V"])
    line = {"tool": "spares_bench", "n": a.n, "units": a.units, "draws": a.draws, "batch": a.batch, "nh": H,
            "horizons": h.tolist(), "ok": ok, "bit_equal_to_restatement_on_slice": bool(same),
            "delta_and_dsum_equal_conditions": same_d, "slice": {"units": cu, "draws": cd},
            "draws_are": "bd_exit(n), every rate times exp(0.15 N(0, 1))",
            "device_ms_per_call": {"median": float(np.median(tot)), "min": float(np.min(tot)),
                                   "max": float(np.max(tot)), "repeats": len(tot), "all": tot},
            "vectors_and_tables_ms_median": med["vec_ms"], "vectors_and_tables_ms_all": t["vec_ms"],
            "unit_ms_median": med["unit_ms"], "unit_ms_all": t["unit_ms"],
            "wall_ms_median": med["wall_ms"], "wall_ms_all": t["wall_ms"],
            "pairs": pairs, "pairs_per_s": pairs / (med["unit_ms"] * 1e-3),
            "condition_device_ms_per_call": {"median": float(np.median(cd_tot)), "min": float(np.min(cd_tot)),
                                             "max": float(np.max(cd_tot)), "all": cd_tot},
            "condition_table_ms_median": med["cd_tab_ms"], "condition_unit_ms_median": med["cd_unit_ms"],
            "condition_wall_ms_median": med["cd_wall_ms"], "condition_wall_ms_all": t["cd_wall_ms"],
            "unit_over_condition_unit": med["unit_ms"] / med["cd_unit_ms"],
            "long_horizon": {"horizons": h_long.tolist(), "mu_h_max_largest": mu_max * float(h_long[-1]),
                             "flagged_draws": int(rl["bad_draw"].sum()), "repeats": a.long_repeats,
                             "vectors_and_tables_ms_median": medl["vec_ms"], "unit_ms_median": medl["unit_ms"],
                             "wall_ms_median": medl["wall_ms"], "condition_table_ms_median": medl["cd_tab_ms"],
                             "condition_unit_ms_median": medl["cd_unit_ms"],
                             "condition_wall_ms_median": medl["cd_wall_ms"], "all": tl},
            "demand_mean": mom["mean"].tolist(), "sd_within": np.sqrt(mom["within"]).tolist(),
            "sd_between": np.sqrt(mom["between"]).tolist(), "sd": mom["sd"].tolist(),
            "lib_key": P.lib_key()}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
