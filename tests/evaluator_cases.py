"""The generators, observations and mpmath truth on which both log-likelihood
evaluators (include/pht_loglik.h, include/pht_loglik_unif.h) are tested off
BD-exit.  Shared by tests/test_loglik.py, test_loglik_unif.py, test_estep.py,
test_quantile.py and the GPU tests of the two kernels; OFF_BD_GPU, fleet and
horizons are the cases and shapes on which the GPU tests of the six
post-processing kernels run the same families, TRUTH_CASES the generators that
test_condition.py, test_spares.py and test_forecast.py add to their own.  CPU
only: no GPU and no oracle is in it.

Families, each (S, s) with pi = e_1:

* ``bd``: bd_exit(n), the generator every earlier test used;
* ``acyclic``, ``reversible``, ``neareq``: the structures of
  tests/test_gpu_structures.py at a perturbed parameter (pathlaw_ref.generator);
* ``stiff``: bd_exit(n) with row i scaled by logspace(-2, 2, n)[i];
* ``erlang``: n phases of one rate (an exactly defective spectrum);
* ``coxian_shared``: every total rate the same, exit probability p before the
  last state (defective as well);
* ``gapped``: an Erlang chain with rates lam (1 + eps i): nearly defective;
* ``hypoexp``: the chain with rates 1 .. n and s_1 = 0 (well conditioned, but
  f(y) ~ y^(n-1) at a small y while the coefficients stay of order one).

Observations: Y_GRID, each exact and censored, without the y beyond
mu y = 1400 (the uniformisation table's cap).

Truth: log f(y) or log Fbar(y) from mpmath.expm at a working precision chosen
per (generator, y): an entry of exp(S y) is as small as y^(n-1) at a small y and
exp(-mu y) at a large one, and expm's error is absolute, so the digits grow
with both.  The Erlang closed forms guard the helper itself.
"""
import math

import numpy as np

from phasetype_amd.synth import bd_exit

Y_GRID = (1e-9, 1e-6, 1e-3, 0.1, 1.0, 5.0, 20.0, 60.0)
MU_Y_MAX = 1400.0
LAM, P_EXIT = 1.3, 0.3
EPS = (1e-12, 1e-9, 1e-6, 1e-3)
NEW_N = (3, 6, 10)
STRUCT_N = (6, 12)


# ---------------------------------------------------------------- generators
def _chain(rates, exit_p=0.0):
    """0 -> 1 -> ... -> n-1 -> absorbed with total rates ``rates``; before the
    last state a fraction exit_p of each rate leaves directly"""
    rates = np.asarray(rates, np.float64)
    n = len(rates)
    S = np.zeros((n, n))
    s = np.zeros(n)
    for i in range(n):
        S[i, i] = -rates[i]
        if i + 1 < n:
            s[i] = rates[i] * exit_p
            S[i, i + 1] = rates[i] - s[i]
        else:
            s[i] = rates[i]
    return S, s


def erlang(n, lam=LAM):
    return _chain(np.full(n, lam))


def coxian_shared(n, lam=LAM, p=P_EXIT):
    return _chain(np.full(n, lam), p)


def gapped(n, lam=LAM, eps=1e-3):
    return _chain(lam * (1.0 + eps * np.arange(n)))


def hypoexp(n):
    return _chain(np.arange(1.0, n + 1.0))


def stiff(n):
    S, s = bd_exit(n)
    c = np.logspace(-2, 2, n)
    return S * c[:, None], s * c


def structure(kind, n):
    import pathlaw_ref as PL

    return PL.generator(kind, n)


def generator(family, n, **kw):
    if family == "bd":
        return bd_exit(n)
    if family in ("acyclic", "reversible", "neareq"):
        return structure(family, n)
    return {"stiff": stiff, "erlang": erlang, "coxian_shared": coxian_shared, "gapped": gapped,
            "hypoexp": hypoexp}[family](n, **kw)


def case_id(case):
    family, n, kw = case
    return "-".join([family, str(n)] + [f"{k}{v:g}" for k, v in sorted(kw.items())])


# (family, n, keyword arguments): every case off BD-exit, and bd itself at the new sizes
CASES = ([("bd", n, {}) for n in NEW_N]
         + [(f, n, {}) for f in ("acyclic", "reversible", "neareq", "stiff") for n in STRUCT_N]
         + [(f, n, {}) for f in ("erlang", "coxian_shared", "hypoexp") for n in NEW_N]
         + [("gapped", n, {"eps": e}) for n in NEW_N for e in EPS])
# one per family for the kernels' bit-exactness (n in NEW_N there, set by the test)
FAMILIES = ("bd", "acyclic", "reversible", "neareq", "stiff", "erlang", "coxian_shared", "gapped", "hypoexp")

# the cases on which the six post-processing kernels (E-step, quantile,
# forecast, condition, spares, predict) run off BD-exit on the GPU: every
# family; n = 3 and 10 take the kernels' compile-time builds, n = 6 and 12 the
# runtime-n ones, and neither of the latter divides the wave
OFF_BD_GPU = ([(f, n, {}) for f in ("acyclic", "reversible", "neareq", "stiff") for n in STRUCT_N]
              + [(f, n, {"eps": 1e-3} if f == "gapped" else {})
                 for f in ("bd", "erlang", "coxian_shared", "gapped", "hypoexp") for n in (3, 10)])
assert len(OFF_BD_GPU) == 18 and {c[0] for c in OFF_BD_GPU} == set(FAMILIES)
DRAW_SCALE = 1.25  # the largest scaling of loglik_unif_ref.SCALES, the five draws of every such test
MU_C_MAX = 1000.0  # the documented limit of an age (README): mu c <= 1000
HORIZON_GRID = (0.0, 1e-9, 1e-3, 0.1, 1.0, 10.0)
QUANTILE_P = (1e-6, 1e-3, 0.1, 0.5, 0.9, 1 - 1e-9)


# -------------------------------------------------------------- observations
def observations(S, scale=1.0):
    """(y, cens): Y_GRID exact, then Y_GRID censored, without the y with
    mu y > MU_Y_MAX for the generator (times ``scale``, its largest scaling)"""
    mu = float(np.max(-np.diag(S))) * scale
    ys = [y for y in Y_GRID if mu * y <= MU_Y_MAX]
    k = len(ys)
    return (np.array(ys + ys), np.concatenate([np.zeros(k, np.int32), np.ones(k, np.int32)]))


def tiled(y, cens, N):
    """N observations: the (y, cens) pairs with exact and censored interleaved,
    repeated, so that every wavefront holds all of them"""
    k = len(y) // 2
    order = np.arange(2 * k).reshape(2, k).T.reshape(-1)  # exact y0, censored y0, exact y1, ...
    idx = order[np.arange(N) % (2 * k)]
    return np.ascontiguousarray(y[idx]), np.ascontiguousarray(cens[idx].astype(np.int32))


# the generators on which tests/test_condition.py, test_spares.py and
# test_forecast.py hold their restatements to the truth, beyond their own five
TRUTH_CASES = {family + str(n): (lambda family=family, n=n, kw=kw: generator(family, n, **kw))
               for family, n, kw in [("acyclic", 6, {}), ("reversible", 6, {}), ("neareq", 6, {}), ("erlang", 6, {}),
                                     ("coxian_shared", 6, {}), ("gapped", 6, {"eps": 1e-9}), ("hypoexp", 6, {}),
                                     ("hypoexp", 10, {}), ("acyclic", 12, {}), ("stiff", 12, {})]}


def fleet(S, scale=DRAW_SCALE, units=65):
    """(y, cens) of a fleet: the ages of Y_GRID with scale mu c <= MU_C_MAX,
    tiled to ``units`` censored units with as many exact observations
    interleaved (exact y0, censored y0, exact y1, ...: ties among the ages and
    between an exact and a censored observation come from the tiling)"""
    mu = float(np.max(-np.diag(S))) * scale
    ages = [c for c in Y_GRID if mu * c <= MU_C_MAX]
    k = len(ages)
    y = np.array(ages + ages)
    cens = np.concatenate([np.zeros(k, np.int32), np.ones(k, np.int32)])
    return tiled(y, cens, 2 * units)


def horizons(S, scale, c_max):
    """HORIZON_GRID without the h with scale mu (c_max + h) > MU_Y_MAX"""
    mu = float(np.max(-np.diag(S))) * scale
    return np.array([h for h in HORIZON_GRID if mu * (float(c_max) + h) <= MU_Y_MAX])


def off_bd_case(case, units=65):
    """(S, s, y, cens, h) of one case of OFF_BD_GPU: the generator, its fleet
    and the horizons for the largest draw (DRAW_SCALE) and the largest age"""
    family, n, kw = case
    S, s = generator(family, n, **kw)
    y, cens = fleet(S, DRAW_SCALE, units)
    return S, s, y, cens, horizons(S, DRAW_SCALE, float(np.max(y[cens != 0])))


# --------------------------------------------------------------------- truth
_EXPM = {}


def _dps(S, y):
    n = S.shape[0]
    mu = float(np.max(-np.diag(S)))
    return int(60 + math.ceil(3 * n * max(0.0, -math.log10(y))) + math.ceil(mu * y / math.log(10.0)))


def _row(S, y):
    """(first row of exp(S y) as mpmath numbers, the precision it was computed at)"""
    import mpmath as mp

    key = (S.tobytes(), S.shape[0], float(y))
    if key not in _EXPM:
        dps = _dps(S, y)
        with mp.workdps(dps):
            E = mp.expm(mp.matrix(S.tolist()) * mp.mpf(float(y)))
            _EXPM[key] = ([E[0, j] for j in range(S.shape[0])], dps)
    return _EXPM[key]


def truth(S, s, y, cens):
    """log f(y) (cens = 0) or log Fbar(y) (cens = 1) of PH(e_1, S) as an mpmath
    number good to more than 30 digits"""
    import mpmath as mp

    S = np.ascontiguousarray(S, np.float64)
    row, dps = _row(S, y)
    with mp.workdps(dps):
        v = mp.fsum(r * mp.mpf(float(c)) for r, c in zip(row, s)) if not cens else mp.fsum(row)
        assert v > mp.mpf(10) ** (30 - dps), ("the working precision does not resolve this value", y, cens, dps)
        return mp.log(v)


def truths(S, s, y, cens):
    return [truth(S, s, float(a), int(c)) for a, c in zip(y, cens)]


def erlang_closed(n, lam, y, cens):
    """log f = n log lam + (n - 1) log y - lam y - log (n - 1)!, and the log of
    the Poisson-sum survival exp(-lam y) sum_{k < n} (lam y)^k / k!"""
    import mpmath as mp

    with mp.workdps(_dps(erlang(n, lam)[0], y)):
        lam, y = mp.mpf(float(lam)), mp.mpf(float(y))
        if not cens:
            return n * mp.log(lam) + (n - 1) * mp.log(y) - lam * y - mp.log(mp.factorial(n - 1))
        return -lam * y + mp.log(mp.fsum((lam * y) ** k / mp.factorial(k) for k in range(n)))


def ulp(x):
    return float(np.spacing(abs(float(x))))


# ------------------------------------------- the spectral evaluator's contract
# PHT_LL_G and PHT_LL_EMAX of include/pht_loglik.h (test_loglik.py checks that
# the header says the same)
G, E_MAX = 361.0, 2.0 ** -20


def spectral_A(blk, y, cens):
    """A = sum_i |c_i| e_i / sum_i c_i e_i of every observation, in numpy from
    an unflagged block (inf where the sum is not positive)"""
    w = np.ascontiguousarray(blk, np.uint8).view(np.float64)
    n = (len(w) - 2) // 3
    dl, a, b = w[2:2 + n], w[2 + n:2 + 2 * n], w[2 + 2 * n:]
    out = np.full(len(y), np.inf)
    for k, (yi, ci) in enumerate(zip(y, cens)):
        c = b if ci else a
        e = np.exp(dl * yi)
        acc = float(np.sum(c * e))
        if acc > 0:
            out[k] = float(np.sum(np.abs(c) * e)) / acc
    return out


def spectral_bound(A, l):
    """E(A, l) = G 2^-52 A + 1e-13 |l| + ulp(l)"""
    return G * 2.0 ** -52 * A + 1e-13 * abs(float(l)) + ulp(l)
