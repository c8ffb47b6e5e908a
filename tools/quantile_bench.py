#!/usr/bin/env python3
"""Time of pht_ctx_quantile (include/pht_quantile.h) at n = 10, 4096 draws and
P = 3, 99 and 1024 probabilities, from one run on one box:

* the device time per call of its two parts separately (HIP events on the
  context's stream, pht_ctx_quantile_ms): the table kernel and the searches,
  summed over the call's batches; median of --repeats calls after a warm-up
  call, with the range of their sum;
* the evaluations per root (mean and largest) and the flags met;
* the CPU restatement (tests/quantile_spec.c) on one core over a slice of the
  draws, scaled linearly to all of them, for the ratio; its results on the
  slice must be the device's bit for bit.

The draws are bd_exit(n) with every rate scattered log-normally (sigma 0.15)
around its value, the probabilities (k - 1/2) / P for P = 99 and 1024 and the
B10 life, the median and the 99th percentile for P = 3.  Prints one JSON line
and writes it to --out.  Run on the GPU box."""
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


def scattered(n, draws, sigma=0.15, seed=12):
    S, s = bd_exit(n)
    rng = np.random.default_rng(seed)
    Ss, ss = [], []
    for _ in range(draws):
        A = S * np.exp(sigma * rng.standard_normal(S.shape))
        b = s * np.exp(sigma * rng.standard_normal(s.shape))
        np.fill_diagonal(A, 0.0)
        np.fill_diagonal(A, -(A.sum(1) + b))
        Ss.append(A)
        ss.append(b)
    return Ss, ss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--draws", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--given", type=float, default=0.0)
    ap.add_argument("--tmax", type=float, default=None, help="the horizon (default: the table cap's)")
    ap.add_argument("--cpu-draws", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r12", "quantile", "quantile_bench.json"))
    a = ap.parse_args()
    if P.device_count() < 1:
        raise SystemExit("quantile_bench needs a HIP device: " + P.load().pht_last_error().decode())
    import quantile_ref as Q

    Q.spec()
    Ss, ss = scattered(a.n, a.draws)
    sw = P.Sweeper(a.n, P.METHODS["ECS"], 1)
    rows, ok = [], True
    for P_ in (3, 99, 1024):
        probs = np.array([0.1, 0.5, 0.99]) if P_ == 3 else (np.arange(P_) + 0.5) / P_
        r = sw.quantile(Ss, ss, probs, given=a.given, tmax=a.tmax, batch=a.batch)  # warm-up
        ms, tab_ms, sea_ms = [], [], []
        for _ in range(a.repeats):
            sw.quantile(Ss, ss, probs, given=a.given, tmax=a.tmax, batch=a.batch)
            tab_ms.append(float(sw.last_quantile_ms[0]))
            sea_ms.append(float(sw.last_quantile_ms[1]))
            ms.append(tab_ms[-1] + sea_ms[-1])
        Dc = min(a.cpu_draws, a.draws)
        t0 = time.perf_counter()
        w = Q.quantile(Ss[:Dc], ss[:Dc], probs, given=a.given, tmax=np.inf if a.tmax is None else a.tmax)
        cpu_s = time.perf_counter() - t0
        same = all(np.array_equal(np.ascontiguousarray(r[k][:Dc]).view(np.uint8),
                                  np.ascontiguousarray(w[k]).view(np.uint8)) for k in ("t", "lo", "hi", "nev", "flags"))
        ok = ok and same and not r["flags"].any() and bool(np.all(np.isfinite(r["t"])))
        med = float(np.median(ms))
        roots = a.draws * P_
        rows.append({
            "P": P_, "roots": roots, "ok": bool(same),
            "device_ms_per_call": {"median": med, "min": float(np.min(ms)), "max": float(np.max(ms)),
                                   "repeats": len(ms), "all": ms},
            "table_ms_median": float(np.median(tab_ms)), "search_ms_median": float(np.median(sea_ms)),
            "search_ns_per_root": 1e6 * float(np.median(sea_ms)) / roots,
            "ns_per_root": 1e6 * med / roots, "us_per_draw": 1e3 * med / a.draws,
            "evaluations_per_root": {"mean": float(r["nev"].mean()), "max": int(r["nev"].max())},
            "flagged_roots": int((r["flags"] != 0).sum()),
            "cpu_restatement_one_core": {"s": cpu_s, "draws": Dc, "scaled_s": cpu_s * a.draws / Dc,
                                         "gpu_speedup": cpu_s * a.draws / Dc / (med * 1e-3)},
        })
    sw.close()
    Ks = [Q.meta(S, s, np.inf if a.tmax is None else a.tmax)["K"] for S, s in zip(Ss, ss)]
    line = {"tool": "quantile_bench", "n": a.n, "draws": a.draws, "batch": a.batch, "given": a.given, "tmax": a.tmax,
            "ok": ok, "draws_are": "bd_exit(n), every rate times exp(0.15 N(0, 1))",
            "K": [min(Ks), max(Ks)], "rows": rows,
            "lib_key": P.lib_key()}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
