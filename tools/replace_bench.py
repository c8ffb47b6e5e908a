#!/usr/bin/env python3
"""Time of pht_ctx_replace (include/pht_replace.h) at n = 10: 4000 draws x 256
ages x 4 cost pairs, from one run on one box:

* the device time per call of its two parts separately (HIP events on the
  context's stream, pht_ctx_replace_ms): the tables with the curve, and the
  policies, summed over the call's batches; median of --repeats calls after a
  warm-up call, with the range of their sum;
* the device time per refined root, the points evaluated per root and the flags
  met; beside it, from the same session, the quantile kernel's device time per
  root on the same draws (99 probabilities), the one-lane search the wave
  multisection is to be compared with;
* replace_host (pht_replace_host, one core) over a slice of the same call,
  scaled linearly to all draws, for the ratio; its results on the slice must be
  the device's bit for bit.

The draws are bd_exit(n) with every rate scattered log-normally (sigma 0.15)
around its value, the ages 256 geometric points from 0.02 to 8 times the median
mean life, the pairs (1, 3), (1, 10), (1, 30) and (1, 100).  No speed threshold
is set.  Prints one JSON line and writes it to --out.  Run on the GPU box."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import phasetype_amd as P  # noqa: E402
from quantile_bench import scattered  # noqa: E402

KEYS = ("t", "g", "lo", "hi", "j", "nev", "flags", "lS", "lf", "M", "age_flags")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--draws", type=int, default=4000)
    ap.add_argument("--ages", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cpu-draws", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r35", "replace", "replace_bench.json"))
    a = ap.parse_args()
    if P.device_count() < 1:
        raise SystemExit("replace_bench needs a HIP device: " + P.load().pht_last_error().decode())
    Ss, ss = scattered(a.n, a.draws)
    m = np.median([np.linalg.solve(-S, np.ones(a.n))[0] for S in Ss])
    ages = m * np.geomspace(0.02, 8.0, a.ages)
    cp, cf = np.ones(4), np.array([3.0, 10.0, 30.0, 100.0])
    sw = P.Sweeper(a.n, P.METHODS["ECS"], 1)
    r = sw.replace(Ss, ss, ages, cp, cf, batch=a.batch, pointwise=True)  # warm-up
    ms, cur_ms, pol_ms = [], [], []
    for _ in range(a.repeats):
        sw.replace(Ss, ss, ages, cp, cf, batch=a.batch)
        cur_ms.append(float(sw.last_replace_ms[0]))
        pol_ms.append(float(sw.last_replace_ms[1]))
        ms.append(cur_ms[-1] + pol_ms[-1])
    # the quantile kernel on the same draws, the same session
    probs = (np.arange(99) + 0.5) / 99
    q = sw.quantile(Ss, ss, probs, batch=a.batch)
    q_ms = []
    for _ in range(a.repeats):
        sw.quantile(Ss, ss, probs, batch=a.batch)
        q_ms.append(float(sw.last_quantile_ms[1]))
    sw.close()
    Dc = min(a.cpu_draws, a.draws)
    t0 = time.perf_counter()
    host = [P.replace_host(Ss[d], ss[d], ages, cp, cf) for d in range(Dc)]
    cpu_s = time.perf_counter() - t0
    same = all(np.array_equal(np.ascontiguousarray(r[k][d]).view(np.uint8),
                              np.ascontiguousarray(host[d][k]).view(np.uint8)) for k in KEYS for d in range(Dc))
    refined = int((r["nev"] > 0).sum())
    med, pol = float(np.median(ms)), float(np.median(pol_ms))
    flags, counts = np.unique(r["flags"], return_counts=True)
    line = {
        "tool": "replace_bench", "n": a.n, "draws": a.draws, "ages": a.ages, "pairs": 4, "batch": a.batch,
        "ok": bool(same) and not bool(r["bad_draw"].any()),
        "draws_are": "bd_exit(n), every rate times exp(0.15 N(0, 1))",
        "device_ms_per_call": {"median": med, "min": float(np.min(ms)), "max": float(np.max(ms)), "repeats": len(ms),
                               "all": ms},
        "curve_ms_median": float(np.median(cur_ms)), "policy_ms_median": pol,
        "curve_ns_per_point": 1e6 * float(np.median(cur_ms)) / (a.draws * a.ages),
        "refined_roots": refined, "policy_ns_per_refined_root": 1e6 * pol / max(refined, 1),
        "points_per_refined_root": {"mean": float(r["nev"][r["nev"] > 0].mean()) if refined else 0.0,
                                    "max": int(r["nev"].max())},
        "flags": {str(int(f)): int(c) for f, c in zip(flags, counts)},
        "bad_ages": int((r["age_flags"] != 0).sum()),
        "quantile_same_session": {"P": 99, "search_ms_median": float(np.median(q_ms)),
                                  "search_ns_per_root": 1e6 * float(np.median(q_ms)) / (a.draws * 99),
                                  "evaluations_per_root_mean": float(q["nev"].mean())},
        "replace_host_one_core": {"s": cpu_s, "draws": Dc, "scaled_s": cpu_s * a.draws / Dc,
                                  "gpu_speedup": cpu_s * a.draws / Dc / (med * 1e-3)},
        "lib_key": P.lib_key(),
    }
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
