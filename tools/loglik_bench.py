#!/usr/bin/env python3
"""Time of pht_ctx_loglik (accumulate mode: totals + WAIC state, the
production path) at n = 10, N = 10^6, 256 draws in batches of 64, next to
the two figures it is read against, on the same box:

* one ECS sweep kernel at the same (n, N) (HIP events, pht_gibbs_run), and
* the CPU restatement of include/pht_loglik.h (tests/loglik_spec.c) on one
  core, timed at 10^4 observations x 16 draws and scaled linearly.

The log-likelihood time is the device time of the call's kernel launches (HIP
events on the context's stream, pht_ctx_last_kernel_ms), median of --repeats
calls after a warm-up call.  The FP64-VALU fraction is implied: FP64
operations counted from the specification (flops_per_eval, fma = 2) over
that time and the MI355X's 78.6 TFLOP/s FP64 vector peak; no counter is read.
Prints one JSON line and writes it to --out.  Run on the GPU box.

--evaluator unif times pht_ctx_loglik_unif (include/pht_loglik_unif.h) instead,
on ring(n) draws (bd_exit(n) with a rate 1.5 from state n back to state 1: a
complex spectrum) scaled 0.8 .. 1.25, with the spectral evaluator timed in the
same run on bd_exit(n) draws over the same observations as the comparison
point; it reports the mean and largest summation window (the CPU restatement on
a sample of observations).  The table kernel's share of the device time is read
from a kernel trace of this tool (rocprofv3 --kernel-trace --stats):
llunif_table_kernel against llunif_kernel."""
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
from phasetype_amd.synth import DATA_KEY, bd_exit, bd_exit_structure, simulate_ph  # noqa: E402

FP64_VALU_PEAK_TF = 78.6  # MI355X FP64 vector peak (bench.py)


def flops_per_eval(n: int, accumulate: bool) -> int:
    """FP64 operations of one (observation, draw) in include/pht_loglik.h,
    fma = 2, min/max/ldexp/rint = 1, integer work and selects not counted.
    pht_exp: clamp 2, shifter fma 2, kd 1, two reduction fma 4, four Horner
    fma 8, r*r 1, two fma 4, add 1, ldexp 1 = 24; a term adds dl*y 1 and the
    chain's fma 2.  pht_log: 32.  finish fma 2, fixed point 3.  WAIC update:
    u, S1, S2 4; the exponent 1, pht_exp 24, r 2."""
    exp = 24
    return n * (exp + 3) + 32 + 2 + 3 + ((4 + 1 + exp + 2) if accumulate else 0)


def _device_ms(sw, call, repeats):
    """median-of-repeats device time of call() after a warm-up, WAIC state reset before each"""
    sw.waic_reset()
    r = call()
    ms = []
    for _ in range(repeats):
        sw.waic_reset()
        call()
        ms.append(float(sw.last_kernel_ms()))
    return r, ms


def bench_unif(a, S, s, y, cen, scales, blocks):
    import loglik_unif_ref as U

    n, N = a.n, a.N
    Sr, sr = U.ring(n)
    Ss, ss = [Sr * c for c in scales], [sr * c for c in scales]
    sw = P.Sweeper(n, P.METHODS["ECS"], 1)
    sw.set_obs(y, cen)
    r, unif_ms = _device_ms(sw, lambda: sw.loglik_unif(Ss, ss, batch=a.batch, accumulate=True), a.repeats)
    ok = bool(np.all(np.isfinite(r["total"])) and np.all(r["nobs"] == N))
    rs, spec_ms = _device_ms(sw, lambda: sw.loglik_blocks(blocks, batch=a.batch, accumulate=True), a.repeats)
    ok = ok and bool(np.all(np.isfinite(rs["total"])))
    Ks = [sw.loglik_unif_K(float(np.max(-np.diag(Sk)))) for Sk in Ss]
    sw.close()
    # window lengths: the restatement on every 1000th observation (sorted), every 16th draw
    ys = np.sort(y)[::1000]
    _, khi = U.pointwise(Ss[::16], ss[::16], ys, np.zeros(len(ys), np.int32), ymax=y.max(), with_khi=True)
    klo = np.zeros_like(khi)
    for d, (Sk, sk) in enumerate(zip(Ss[::16], ss[::16])):  # the lower end: the same rule, walked here
        t = U.table(Sk, sk, y.max())
        for i, yi in enumerate(ys):
            lam = t["mu"] * yi
            k0 = min(int(np.floor(lam)), t["K"])
            w, num, k = 1.0, t["tab"][k0, 0], k0
            while k > 0:
                w *= k / lam
                k -= 1
                if w < 2.0 ** -60 and w * t["abar"] < 2.0 ** -60 * num:
                    k += 1
                    break
                num += w * t["tab"][k, 0]
            klo[d, i] = k
    win = (khi - klo + 1).astype(np.float64)
    med, smed = float(np.median(unif_ms)), float(np.median(spec_ms))
    line = {
        "tool": "loglik_bench", "evaluator": "unif", "n": n, "N": N, "draws": a.draws, "batch": a.batch,
        "mode": "accumulate", "ok": ok, "draws_are": "ring(n) scaled 0.8..1.25", "K": [min(Ks), max(Ks)],
        "device_ms_per_call": {"median": med, "min": float(np.min(unif_ms)), "max": float(np.max(unif_ms)),
                               "repeats": len(unif_ms), "all": unif_ms},
        "device_us_per_draw": 1e3 * med / a.draws,
        "spectral_same_run": {"draws_are": "bd_exit(n) scaled 0.8..1.25", "device_ms_per_call_median": smed,
                              "device_us_per_draw": 1e3 * smed / a.draws, "all": spec_ms},
        "unif_over_spectral": med / smed,
        "window": {"mean": float(win.mean()), "max": int(win.max()), "sample": list(win.shape),
                   "note": "terms summed per (observation, draw); exact observations"},
        "lib_key": P.lib_key(),
    }
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(line, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--N", type=int, default=1_000_000)
    ap.add_argument("--draws", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sweeps", type=int, default=24, help="ECS sweeps of the comparison run")
    ap.add_argument("--evaluator", choices=("spectral", "unif"), default="spectral")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = (os.path.join(REPO, "profiles", "r07", "loglik", "loglik_bench.json") if a.evaluator == "spectral"
                 else os.path.join(REPO, "profiles", "r08", "loglik_unif", "loglik_unif_bench.json"))
    if P.device_count() < 1:
        raise SystemExit("loglik_bench needs a HIP device: " + P.load().pht_last_error().decode())
    n, N = a.n, a.N
    S, s = bd_exit(n)
    y, cen = simulate_ph(S, s, N, seed=DATA_KEY, censor_frac=0.0)
    scales = np.linspace(0.8, 1.25, a.draws)
    blocks = np.stack([P.loglik_block(S * c, s * c) for c in scales])
    if a.evaluator == "unif":
        return bench_unif(a, S, s, y, cen, scales, blocks)

    sw = P.Sweeper(n, P.METHODS["ECS"], 1)
    sw.set_obs(y, cen)
    sw.waic_reset()
    r = sw.loglik_blocks(blocks, batch=a.batch, accumulate=True)  # warm-up
    ok = bool(np.all(np.isfinite(r["total"])) and np.all(r["nobs"] == N))
    dev_ms, wall_ms = [], []
    for _ in range(max(5, a.repeats)):
        sw.waic_reset()
        t0 = time.perf_counter()
        sw.loglik_blocks(blocks, batch=a.batch, accumulate=True)
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(float(sw.last_kernel_ms()))
    # totals only (no WAIC state traffic), for the difference
    tot_ms = []
    for _ in range(5):
        sw.loglik_blocks(blocks, batch=a.batch)
        tot_ms.append(float(sw.last_kernel_ms()))

    # the ECS sweep kernel at the same (n, N), as tools/resident_bench.py times it
    T, theta = bd_exit_structure(n)
    nu, zeta, Cm = 1 + 50 * theta, np.full(len(theta), 50.0), np.ones(T.shape)
    zexp = P.zexp_for(y)
    P.set_seed(1)
    w = sw.gibbs(3, P.METHODS["ECS"], nu, zeta, T, Cm, zexp)
    os.environ["PHT_KTIME_EVERY"] = "1"
    sw.gibbs(a.sweeps + 1, P.METHODS["ECS"], nu, zeta, T, Cm, zexp, start=w[-1])
    ecs_ms = sw.kernel_ms_total / a.sweeps
    sw.close()

    # the restatement on one core
    import loglik_ref as R

    Nc, Dc = 10_000, 16
    R.spec()
    t0 = time.perf_counter()
    lc = R.pointwise(blocks[:Dc], y[:Nc], cen[:Nc])
    R.totals(lc)
    R.waic_state(lc)
    cpu_s = time.perf_counter() - t0
    cpu_scaled_s = cpu_s * (N / Nc) * (a.draws / Dc)

    med = float(np.median(dev_ms))
    flops = flops_per_eval(n, True) * float(N) * a.draws
    tfs = flops / (med * 1e-3) / 1e12
    line = {
        "tool": "loglik_bench", "n": n, "N": N, "draws": a.draws, "batch": a.batch, "mode": "accumulate", "ok": ok,
        "device_ms_per_call": {"median": med, "min": float(np.min(dev_ms)), "max": float(np.max(dev_ms)),
                               "repeats": len(dev_ms), "all": dev_ms},
        "device_ms_per_draw": med / a.draws,
        "wall_ms_per_call_median": float(np.median(wall_ms)),
        "totals_only_device_ms_per_call_median": float(np.median(tot_ms)),
        "fp64_valu_implied": {"flops_per_eval": flops_per_eval(n, True), "achieved_tflops": tfs,
                              "peak_tflops": FP64_VALU_PEAK_TF, "frac": tfs / FP64_VALU_PEAK_TF,
                              "note": "operations counted from the specification (fma = 2), not a counter"},
        "ecs_sweep_kernel_ms": ecs_ms, "ecs_sweeps_timed": a.sweeps,
        "draw_over_ecs_sweep": (med / a.draws) / ecs_ms,
        "cpu_restatement_one_core": {"measured_s": cpu_s, "at": [Nc, Dc], "scaled_s": cpu_scaled_s,
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
