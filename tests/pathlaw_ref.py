"""The path law of every sampler against exact expectations, off BD-exit: the
generators, observation layout, truths, checks and the case table shared by
tests/test_pathlaw.py (the oracle's device specification, CPU) and
tests/test_gpu_pathlaw.py (the HIP kernels' own records).  CPU only: the
truth comes from the E-step restatement (tests/estep_ref.py, itself checked
against mpmath at 50 digits) and the quantile restatement
(tests/quantile_ref.py); neither the GPU nor the oracle is in it.

A case is one (generator, sampler, mode) at the times where PH(e_1, S) has
F(y) = 0.01, 0.5, 0.99 and 0.9999, each exact and censored, R replicates per
(y, censoring) group, the groups interleaved so that every wavefront mixes
short and long, exact and censored paths.  Three checks per case:

* ``invariants``: the deterministic bookkeeping of a sampled path;
* ``group_zscores``: per group and cell |mean - truth| / se against
  E[z | y], E[N | y], E[exits | y] of the completed path;
* ``residual_life``: the part of a censored path beyond y against the
  residual-life quantiles.
"""
import numpy as np

import estep_ref as ER
import quantile_ref as QR
import test_gpu_structures as TS
from oracle.posterior import K_SIGMA
from phasetype_amd import complete_stats
from phasetype_amd.synth import bd_exit

PROBS = (0.01, 0.5, 0.99, 0.9999)
RES_P = np.array([0.1, 0.5, 0.9])
ECS, MHRS, DCS, UNIF = 2, 1, 4, 8


# ---------------------------------------------------------------- generators
def cyclic(n, holes=False, seed=0):
    """tests/test_gpu_bridge.py's ring 0 -> 1 -> ... -> n-1 -> 0 with weak
    back-steps (a complex spectrum); ``holes``: every second exit rate 0."""
    rng = np.random.default_rng(seed)
    S = np.zeros((n, n))
    for i in range(n):
        S[i, (i + 1) % n] = rng.uniform(1.5, 3.0)
        S[i, (i - 1) % n] += rng.uniform(0.0, 0.2)
    s = rng.uniform(0.1, 0.5, n)
    if holes:
        s[1::2] = 0.0
    np.fill_diagonal(S, 0.0)
    np.fill_diagonal(S, -(S.sum(1) + s))
    return S, s


def generator(kind, n):
    """(S, s) of a case: the structures of tests/test_gpu_structures.py at a
    perturbed parameter (as its parity cases run them), the rings, BD-exit"""
    if kind == "bd":
        return bd_exit(n)
    if kind in ("cyclic", "holes"):
        return cyclic(n, holes=kind == "holes")
    S0, s0 = TS.generator(kind, n, 100 + n)
    return TS.sweep_params(kind, S0, s0, 7 * n + 1)


def ygrid(S, s, probs=PROBS):
    """the times t with F(t) = probs for PH(e_1, S), from the CPU restatement"""
    r = QR.quantile([S], [s], np.asarray(probs, np.float64))
    assert not r["bad_draw"][0] and not r["flags"][0].any() and np.all(np.diff(r["t"][0]) > 0)
    return r["t"][0].copy()


def layout(ys, R, cens=(0, 1)):
    """(y, censored, group of each observation, [(y, c) per group]): all
    (y, c) pairs R times, observation i in group i % ngroups"""
    pairs = [(float(yv), int(c)) for yv in ys for c in cens]
    G = len(pairs)
    grp = np.arange(G * R) % G
    y = np.array([p[0] for p in pairs])[grp]
    cen = np.array([p[1] for p in pairs], np.int32)[grp]
    return np.ascontiguousarray(y), np.ascontiguousarray(cen), grp, pairs


# --------------------------------------------------------------------- truth
def truth(S, s, y, cens):
    """(Z [n], N [n, n]) of one observation's completed path: E[z_i | y] and
    E[N_ij | y] with the expected exits on the diagonal (a sweep block's
    layout); cens = 1 conditions on Y > y and runs on to absorption"""
    r = ER.estep(S, s, np.array([y]), np.array([cens], np.int32))
    assert r["flag"] == 0 and r["nbad"] == 0
    Z, N, E = complete_stats(S, s, r["Z"], r["N"], r["E"], r["A"])
    return Z, N + np.diag(E)


def case_truths(S, s, pairs, method):
    """truth per group; DCS (native and bridge) treats a censored observation
    as exact (src/Simulate_AbsCTMC_eq_AslettHobolth_DCS.c:132-133)"""
    memo = {}
    out = []
    for yv, c in pairs:
        k = (yv, 0 if method == DCS else c)
        if k not in memo:
            memo[k] = truth(S, s, *k)
        out.append(memo[k])
    return out


# -------------------------------------------------------------------- checks
def _cell_z(mean, want, var, R):
    se = np.sqrt(var / R)
    d = np.abs(mean - want)
    z = np.where(se > 0, d / np.where(se > 0, se, 1.0), np.where(d > 0, np.inf, 0.0))
    # a cell whose truth is 0 must have mean exactly 0
    return np.where(want == 0, np.where(mean == 0, 0.0, np.inf), z), se


def group_zscores(zq, zexp, N, groups, truths, S):
    """Per group and cell |mean - truth| / se with the floors of
    test_oracle_ref._check_expectations (variance of z >= E / -S_ii, of a
    count >= E).  dict(z [G, n], N [G, n, n], worst, detect): ``detect`` is
    5 se of the worst cell, the smallest bias the bar sees there."""
    S = np.asarray(S, np.float64)
    G, n = len(truths), S.shape[0]
    zz, zN = np.zeros((G, n)), np.zeros((G, n, n))
    worst, detect = -1.0, 0.0
    for g in range(G):
        sel = groups == g
        R = int(sel.sum())
        Ez, EN = truths[g]
        z = np.ldexp(zq[sel].astype(np.float64), -int(zexp))
        zz[g], sez = _cell_z(z.mean(0), Ez, np.maximum(z.var(0), np.abs(Ez) / -np.diag(S)), R)
        Ng = N[sel].astype(np.float64)
        zN[g], seN = _cell_z(Ng.mean(0), EN, np.maximum(Ng.var(0), np.abs(EN)), R)
        for zs, se in ((zz[g], sez), (zN[g], seN)):
            k = np.unravel_index(np.argmax(zs), zs.shape)
            if zs[k] > worst:
                worst, detect = float(zs[k]), float(K_SIGMA * se[k])
    return dict(z=zz, N=zN, worst=worst, detect=detect)


def invariants(rec, S, y, cens, method, s=None):
    """The bookkeeping of every sampled path of a sweep_debug / dev_sweep
    record (with its ``zexp``): a list of "name: first offending
    observations", empty when all hold."""
    S = np.asarray(S, np.float64)
    n = S.shape[0]
    N, zq, pre = rec["N"].astype(np.int64), rec["zq"], np.asarray(rec["pre"], np.int64)
    eye = np.eye(n, dtype=bool)
    diag = np.diagonal(N, axis1=1, axis2=2)
    off = np.where(eye[None], 0, N)
    exits = off.sum(2) + diag
    entries = off.sum(1)
    entries = entries + (np.arange(n)[None, :] == np.asarray(rec["B"])[:, None])
    bad = {}
    bad["flow: entries + [i = B] != exits"] = np.any(entries != exits, axis=1)
    bad["absorption: diagonal of N does not sum to 1"] = diag.sum(1) != 1
    inr = (pre >= 0) & (pre < n)
    bad["pre is not the exit state"] = ~inr | (diag[np.arange(len(pre)), np.where(inr, pre, 0)] != 1)
    bad["B != 0"] = np.asarray(rec["B"]) != 0
    forbidden = (S <= 0) & ~eye
    if s is not None:
        forbidden = forbidden | (eye & (np.asarray(s)[:, None] <= 0))
    bad["count where the rate is 0"] = np.any(N[:, forbidden] != 0, axis=1)
    bad["zq < 0"] = np.any(zq < 0, axis=1)
    bad["time in a state the path never left"] = np.any((zq != 0) & (exits == 0), axis=1)
    bad["flags != 0"] = np.asarray(rec["flags"]) != 0
    tot = np.ldexp(zq.sum(1).astype(np.float64), -int(rec["zexp"]))
    bound = (N.sum(axis=(1, 2)) + 2) * 2.0 ** -int(rec["zexp"]) + 1e-13 * y
    exact = (np.asarray(cens) == 0) | (method == DCS)
    bad["sum z != y (exact)"] = exact & (np.abs(tot - y) > bound)
    bad["sum z < y (censored)"] = ~exact & (tot < y - bound)
    return [f"{k}: obs {np.nonzero(v)[0][:5].tolist()}" for k, v in bad.items() if v.any()]


def residual_life(tot, y, S, s, given=None):
    """A censored group's sum z - y against the residual-life quantiles q_p,
    p = 0.1, 0.5, 0.9 (tests/quantile_ref.py, given = y): the counts at or
    below q_p in standard deviations sqrt(R p (1 - p)) from R p; the bar is 5
    (tests/test_gpu_quantile.py test_against_rph's)."""
    r = QR.quantile([S], [s], RES_P, given=float(y if given is None else given))
    assert not r["bad_draw"][0] and not r["flags"][0].any()
    rest = np.asarray(tot, np.float64) - y
    R = len(rest)
    cnt = np.array([(rest <= q).sum() for q in r["t"][0]])
    return (cnt - R * RES_P) / np.sqrt(R * RES_P * (1 - RES_P))


def check_record(rec, case, S, s, lay, truths):
    """the three checks of one case's record: dict(violations, worst,
    detect, resid) with ``resid`` the largest residual-life deviation"""
    y, cen, grp, pairs = lay
    viol = invariants(rec, S, y, cen, case["method"], s)
    zs = group_zscores(rec["zq"], rec["zexp"], rec["N"], grp, truths, S)
    resid = 0.0
    if case["method"] != DCS:  # exact-law samplers: the censored path goes on beyond y
        tot = np.ldexp(rec["zq"].sum(1).astype(np.float64), -int(rec["zexp"]))
        for g, (yv, c) in enumerate(pairs):
            if c:
                resid = max(resid, float(np.abs(residual_life(tot[grp == g], yv, S, s)).max()))
    return dict(violations=viol, worst=zs["worst"], detect=zs["detect"], resid=resid, z=zs)


# ---------------------------------------------------------------- case table
def _case(name, method, kind, n, key, sweep, mhit=1, probs=PROBS, cens=(0, 1), env=None, bridge=None,
          general=False):
    return dict(name=name, method=method, kind=kind, n=n, R=2000 if n >= 15 else 4000, key=key, sweep=sweep,
                mhit=mhit, probs=probs, cens=cens, env=env or {}, bridge=bridge, general=general)


P3 = PROBS[:3]
CASES = [
    # ECS; the two BD-exit cases' tail groups drive the general ARMS code and the private envelope, counted
    # by the one-lane blocks' debug launch (hence no rows there)
    _case("ecs-acyclic8", ECS, "acyclic", 8, (0x5101, 0x11), 1),
    _case("ecs-acyclic20", ECS, "acyclic", 20, (0x5102, 0x12), 2),  # two spectral indices per lane
    _case("ecs-reversible5", ECS, "reversible", 5, (0x5103, 0x13), 3),
    _case("ecs-reversible10", ECS, "reversible", 10, (0x5104, 0x14), 4),
    _case("ecs-neareq6", ECS, "neareq", 6, (0x5105, 0x15), 5),
    _case("ecs-bd10", ECS, "bd", 10, (0x5106, 0x16), 6, env={"PHT_ROWK": "0"}, general=True),
    _case("ecs-bd15", ECS, "bd", 15, (0x5107, 0x17), 7, env={"PHT_ROWK": "0"}, general=True),
    # ECS with every exact observation on a 16-lane row
    _case("ecsrows-reversible10", ECS, "reversible", 10, (0x5104, 0x14), 4, env={"PHT_ROWK": str(10 ** 9)}),
    _case("ecsrows-acyclic20", ECS, "acyclic", 20, (0x5102, 0x12), 2, env={"PHT_ROWK": str(10 ** 9)}),
    # DCS (censored observations treated as exact)
    _case("dcs-acyclic8", DCS, "acyclic", 8, (0x5201, 0x21), 1),
    _case("dcs-acyclic16", DCS, "acyclic", 16, (0x5202, 0x22), 2),
    _case("dcs-reversible5", DCS, "reversible", 5, (0x5203, 0x23), 3),
    _case("dcs-neareq6", DCS, "neareq", 6, (0x5204, 0x24), 4),  # q5's 1e-13 switch
    _case("dcsprepass-reversible5", DCS, "reversible", 5, (0x5203, 0x23), 3, env={"PHT_DCS_PREPASS": "1"}),
    # UNIF
    _case("unif-acyclic8", UNIF, "acyclic", 8, (0x5301, 0x31), 1),
    _case("unif-reversible15", UNIF, "reversible", 15, (0x5302, 0x32), 2),
    _case("unif-cyclic6", UNIF, "cyclic", 6, (0x5303, 0x33), 3),
    _case("unif-cyclic12", UNIF, "cyclic", 12, (0x5304, 0x34), 4),
    _case("unif-holes6", UNIF, "holes", 6, (0x5305, 0x35), 5),
    # the bridge modes (pht_unif.h ulaw 2 / 1)
    _case("dcsbridge-cyclic6", DCS, "cyclic", 6, (0x5401, 0x41), 1, env={"PHT_DCS": "bridge"}, bridge="dcs"),
    _case("dcsbridge-holes6", DCS, "holes", 6, (0x5402, 0x42), 2, env={"PHT_DCS": "bridge"}, bridge="dcs"),
    _case("dcsbridge-reversible5", DCS, "reversible", 5, (0x5403, 0x43), 3, env={"PHT_DCS": "bridge"},
          bridge="dcs"),
    _case("mhrsbridge-cyclic6", MHRS, "cyclic", 6, (0x5501, 0x51), 1, mhit=25, env={"PHT_MHRS": "bridge"},
          bridge="mhrs"),
    _case("mhrsbridge-reversible5", MHRS, "reversible", 5, (0x5502, 0x52), 2, mhit=25,
          env={"PHT_MHRS": "bridge"}, bridge="mhrs"),
    # native MHRS: the search needs ~1 / density attempts, so no survival-1e-4 time; censored groups are
    # plain rejection (an exact law), exact groups need mhit = 25 (at small mhit biased by design)
    _case("mhrs-acyclic8-cens", MHRS, "acyclic", 8, (0x5601, 0x61), 1, probs=P3, cens=(1,)),
    _case("mhrs-reversible5-cens", MHRS, "reversible", 5, (0x5602, 0x62), 2, probs=P3, cens=(1,)),
    _case("mhrs-reversible5-exact", MHRS, "reversible", 5, (0x5603, 0x63), 3, mhit=25, probs=P3, cens=(0,)),
]
CASE_BY_NAME = {c["name"]: c for c in CASES}

_INPUTS = {}


def inputs(case):
    """(S, s, layout, truths) of a case, computed once per process"""
    k = (case["kind"], case["n"], case["method"], case["probs"], case["cens"], case["R"])
    if k not in _INPUTS:
        S, s = generator(case["kind"], case["n"])
        lay = layout(ygrid(S, s, case["probs"]), case["R"], case["cens"])
        _INPUTS[k] = (S, s, lay, case_truths(S, s, lay[3], case["method"]))
    return _INPUTS[k]


def report(case, res):
    return (f"pathlaw {case['name']}: worst z-score {res['worst']:.2f}, detectable bias {res['detect']:.3g}, "
            f"residual life {res['resid']:.2f} sd")
