#!/usr/bin/env python3
"""When each block of the ECS exact kernel starts, ends its work and ends its
flush (a PHT_BLOCK_TIMES variant build: every one-lane block writes one record,
phasetype_amd/csrc/pht_kernels.h), set against the kernel time by HIP events.

Answers where the gap between the mean wave's life and the dispatch goes:
  1 end times spread with work    rounds per block differ, end ~ rounds
  2 end times spread with speed   rounds even, cycles per round differ (XCD, CU, the CU's other block)
  3 staggered starts              first start -> mean start
  4 drain after the last wave     last end of work -> last end of flush, and what is left outside any wave
  5 none: the working time of the mean block is within 3 % of the kernel time

usage (GPU box):
  python3 tools/build_variant.py blocktimes -D PHT_BLOCK_TIMES
  python3 tools/block_times.py --lib phasetype_amd/_variants/blocktimes.so [--N 1000000 --n 10]
      [--shards W --rank R] [--sweeps 5] [--per-block] [--out profiles/r14/block_times/cfg4.json]
--shards W --rank R: rank R's shard of the real W-GPU partition (its global
ids), as tools/latency.py --shards sweeps them.  Launch knobs (PHT_ECS_OCC,
PHT_SPREAD, PHT_ROWK, ...) are read from the environment as always.
The records perturb nothing inside the rounds (three stamps per block), but
the end-of-flush stamp waits for the block's atomics: read the build's
kernel time beside the default library's before quoting it.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRIEF = ("kernel_ms_events", "decomposition_us", "mean_block_work_over_kernel", "corr_end_rounds",
         "corr_end_cycles_per_round", "corr_end_partner_end")
WALL_HZ = 100e6  # the constant-rate clock of gfx9 (s_memrealtime): 100 MHz


def pct(v):
    q = np.percentile(v, [0, 5, 25, 50, 75, 95, 100])
    return {k: round(float(x), 3) for k, x in zip(("min", "p5", "p25", "p50", "p75", "p95", "max"), q)}


def corr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    if len(a) < 3 or a.std() == 0 or b.std() == 0:
        return None
    return round(float(np.corrcoef(a, b)[0, 1]), 4)


def pair_summary(key, endw, rounds, cpr):
    """CUs holding exactly two blocks: which of the two ends first (blocks in
    launch order, so the lower index is the older one), the two groups' end
    times and speeds, and when each CU's later block ends."""
    order = np.argsort(key, kind="stable")
    ks = key[order]
    first = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    size = np.diff(np.r_[first, len(ks)])
    two = first[size == 2]
    if len(two) == 0:
        return None
    a, b = order[two], order[two + 1]
    old, young = np.minimum(a, b), np.maximum(a, b)
    cu_end = np.maximum(endw[old], endw[young])
    late = np.argsort(-cu_end)[:5]
    q = lambda v: [round(float(x), 1) for x in np.percentile(v, [0, 50, 100])]
    return {"pairs": int(len(two)), "index_offsets": sorted(set((young - old).tolist()))[:4],
            "older_block_ends_first": int((endw[old] < endw[young]).sum()),
            "older_end_of_work_us_min_p50_max": q(endw[old]), "younger_end_of_work_us_min_p50_max": q(endw[young]),
            "older_cycles_per_round_mean": round(float(cpr[old].mean()), 1),
            "younger_cycles_per_round_mean": round(float(cpr[young].mean()), 1),
            "older_rounds_mean": round(float(rounds[old].mean()), 2),
            "younger_rounds_mean": round(float(rounds[young].mean()), 2),
            "cu_end_us_p5_p50_p95_max": [round(float(x), 1) for x in np.percentile(cu_end, [5, 50, 95, 100])],
            "latest_cus_older_block": [int(old[i]) for i in late]}


def analyse(rec, kernel_ms, detail=False):
    """rec: [blocks, words] uint64 records of one sweep; times in microseconds
    from the earliest start."""
    rec = rec[rec[:, 0] != 0]
    nb = len(rec)
    w = rec[:, 0:3].astype(np.int64)
    core = rec[:, 3:6].astype(np.int64)
    t0 = w[:, 0].min()
    us = (w - t0) / WALL_HZ * 1e6
    start, endw, endf = us[:, 0], us[:, 1], us[:, 2]
    rounds = rec[:, 6].astype(np.float64)
    obs = rec[:, 7].astype(np.int64)
    smid = rec[:, 8].astype(np.int64)
    xcc, se, cu = smid >> 6, (smid >> 4) & 3, smid & 15
    cyc = (core[:, 1] - core[:, 0]).astype(np.float64)
    cpr = cyc / np.maximum(rounds, 1.0)
    work = endw - start
    kus = kernel_ms * 1e3
    span = float(endf.max())
    parts = {
        "first_start_to_mean_start": float(start.mean()),
        "mean_start_to_mean_end_of_work": float(endw.mean() - start.mean()),
        "mean_end_of_work_to_last_end_of_work": float(endw.max() - endw.mean()),
        "last_end_of_work_to_last_end_of_flush": float(endf.max() - endw.max()),
        "outside_any_wave": float(kus - span),
    }
    # the CU's other block(s): same (XCC, SE, CU)
    key = (xcc * 4 + se) * 16 + cu
    order = np.argsort(key, kind="stable")
    partner = np.full(nb, -1)
    per_cu = np.bincount(np.unique(key, return_inverse=True)[1])
    i = 0
    while i < nb:
        j = i
        while j + 1 < nb and key[order[j + 1]] == key[order[i]]:
            j += 1
        if j == i + 1:
            partner[order[i]], partner[order[j]] = order[j], order[i]
        i = j + 1
    hasp = partner >= 0
    by_xcc = {}
    for x in sorted(set(xcc.tolist())):
        m = xcc == x
        by_xcc[str(x)] = {"blocks": int(m.sum()), "cus": int(len(set(key[m].tolist()))),
                          "start_us_mean": round(float(start[m].mean()), 3),
                          "end_of_work_us_mean": round(float(endw[m].mean()), 3),
                          "end_of_work_us_max": round(float(endw[m].max()), 3),
                          "rounds_mean": round(float(rounds[m].mean()), 2),
                          "cycles_per_round_mean": round(float(cpr[m].mean()), 1)}
    out = {
        "kernel_ms_events": round(kernel_ms, 5),
        "blocks": nb,
        "observations": int(obs.sum()),
        "core_clock_mhz": round(float(cyc.sum() / np.maximum((w[:, 1] - w[:, 0]).sum(), 1) * WALL_HZ / 1e6), 1),
        "decomposition_us": {k: round(v, 3) for k, v in parts.items()},
        "decomposition_share": {k: round(v / kus, 4) for k, v in parts.items()},
        "span_first_start_to_last_flush_us": round(span, 3),
        "mean_block_work_over_kernel": round(float(work.mean() / kus), 4),
        "no_gap_within_3pct": bool(work.mean() / kus >= 0.97),
        "start_us": pct(start), "end_of_work_us": pct(endw), "end_of_flush_us": pct(endf),
        "flush_us_per_block": pct(endf - endw),
        "rounds_wave0": pct(rounds), "rounds_max_over_mean": round(float(rounds.max() / rounds.mean()), 4),
        "cycles_per_round": pct(cpr), "cycles_per_round_max_over_mean": round(float(cpr.max() / cpr.mean()), 4),
        "observations_per_block": pct(obs),
        "corr_end_rounds": corr(endw, rounds),
        "corr_end_cycles_per_round": corr(endw, cpr),
        "corr_end_start": corr(endw, start),
        "corr_work_rounds": corr(work, rounds),
        "corr_work_cycles_per_round": corr(work, cpr),
        "blocks_per_cu_histogram": {str(k): int(v) for k, v in enumerate(np.bincount(per_cu)) if v},
        "corr_end_partner_end": corr(endw[hasp], endw[partner[hasp]]) if hasp.any() else None,
        "corr_cycles_per_round_partner_rounds": corr(cpr[hasp], rounds[partner[hasp]]) if hasp.any() else None,
        "cu_pairs": pair_summary(key, endw, rounds, cpr),
        "by_xcc": by_xcc,
    }
    if detail:
        out["per_block"] = {"columns": ["block", "xcc", "se", "cu", "partner", "start_us", "end_of_work_us",
                                        "end_of_flush_us", "rounds", "cycles_per_round", "observations"],
                            "rows": [[int(b), int(xcc[b]), int(se[b]), int(cu[b]), int(partner[b]),
                                      round(float(start[b]), 2), round(float(endw[b]), 2), round(float(endf[b]), 2),
                                      int(rounds[b]), round(float(cpr[b]), 1), int(obs[b])] for b in range(nb)]}
    return out


def dumps(out):
    """the summary indented, every sweep (and every per-block row) on one line"""
    head = {k: v for k, v in out.items() if k != "per_sweep"}
    lines = []
    for r in out["per_sweep"]:
        pb = r.get("per_block")
        line = json.dumps({k: v for k, v in r.items() if k != "per_block"})
        if pb:
            rows = ",\n   ".join(json.dumps(x) for x in pb["rows"])
            line = line[:-1] + ', "per_block": {"columns": %s, "rows": [\n   %s]}}' % (json.dumps(pb["columns"]), rows)
        lines.append("  " + line)
    return json.dumps(head, indent=1)[:-2] + ',\n "per_sweep": [\n' + ",\n".join(lines) + "\n ]\n}\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.environ.get("PHT_LIB"), help="the PHT_BLOCK_TIMES variant library")
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--N", type=int, default=1_000_000)
    ap.add_argument("--shards", type=int, default=0)
    ap.add_argument("--rank", type=int, default=0)
    ap.add_argument("--sweeps", type=int, default=5)
    ap.add_argument("--per-block", action="store_true", help="save the last sweep's per-block rows too")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r14", "block_times", "block_times.json"))
    a = ap.parse_args()
    if not a.lib:
        raise SystemExit("block_times.py: give the variant library (--lib or PHT_LIB)")
    os.environ["PHT_LIB"] = os.path.abspath(a.lib)
    sys.path.insert(0, REPO)
    import phasetype_amd as P
    from phasetype_amd.dist import shard_range
    from phasetype_amd.synth import DATA_KEY, bd_exit, simulate_ph

    S, s = bd_exit(a.n)
    y, cen = simulate_ph(S, s, a.N, seed=DATA_KEY)
    lo, hi = shard_range(a.N, a.rank, a.shards) if a.shards else (0, a.N)
    zexp = P.zexp_for(y)
    sw = P.Sweeper(a.n, 2)
    if not hasattr(sw.L, "pht_ctx_block_times"):
        raise SystemExit(f"{a.lib}: not a PHT_BLOCK_TIMES build (tools/build_variant.py NAME -D PHT_BLOCK_TIMES)")
    fn = sw.L.pht_ctx_block_times
    fn.restype = C.c_long
    fn.argtypes = [C.c_void_p, np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS"), C.c_long,
                   C.POINTER(C.c_int)]
    sw.set_obs(np.ascontiguousarray(y[lo:hi]), np.ascontiguousarray(cen[lo:hi]), obs0=lo)
    words = C.c_int()
    fn(sw.ctx, np.zeros(1, np.uint64), 0, C.byref(words))
    cap = 4096
    buf = np.zeros(cap * words.value, np.uint64)
    for k in range(2):  # warm-up
        sw.sweep(S, s, key=(3, 4), sweep=k + 1, zexp=zexp)
    runs = []
    for k in range(a.sweeps):
        sw.sweep(S, s, key=(3, 4), sweep=10 + k, zexp=zexp)
        ms = float(sw.last_kernel_ms())
        got = fn(sw.ctx, buf, cap, C.byref(words))
        if got < 1:
            raise SystemExit("no block records: " + sw.L.pht_last_error().decode())
        runs.append(analyse(buf.reshape(cap, words.value).copy(), ms, detail=(a.per_block and k == a.sweeps - 1)))
    sw.close()
    keys = list(runs[0]["decomposition_us"])
    mean = {k: round(float(np.mean([r["decomposition_us"][k] for r in runs])), 3) for k in keys}
    kus = float(np.mean([r["kernel_ms_events"] for r in runs])) * 1e3
    out = {"n": a.n, "N": a.N, "shard": [int(lo), int(hi)], "lib": os.path.basename(a.lib), "sweeps": a.sweeps,
           "env": {k: v for k, v in os.environ.items() if k.startswith("PHT_") and k != "PHT_LIB"},
           "kernel_us_events_mean": round(kus, 2),
           "decomposition_us_mean": mean,
           "decomposition_share_mean": {k: round(v / kus, 4) for k, v in mean.items()},
           "mean_block_work_over_kernel_mean": round(float(np.mean([r["mean_block_work_over_kernel"] for r in runs])), 4),
           # every sweep's split; the distributions of the last one
           "per_sweep": [{k: r[k] for k in BRIEF} for r in runs[:-1]] + runs[-1:]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(dumps(out))
    brief = dict(out)
    brief["per_sweep"] = [{k: v for k, v in r.items() if k != "per_block"} for r in runs[-1:]]
    print(json.dumps(brief, indent=1))


if __name__ == "__main__":
    main()
