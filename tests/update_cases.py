"""Step 2 of a sweep, the conjugate parameter update, stated in numpy, with the
tied and scaled structures it is tested on and the exact laws its chains must
follow.  Shared by tests/test_update.py (CPU) and tests/test_gpu_update.py;
nothing of oracle/ is imported here.

The statement is written from DESIGN.md §8 (q2) and SURVEY.md §4, not from
the C++: the structure matrices T and C ((n+1)^2; T[i, j] = k + 1 puts
parameter k into cell (i, j) with multiplier C[i, j]) are walked i outer over
rows 0..n, j inner over columns 0..n.  Per parameter k

    Nsum_k = sum over its cells of N[i, j]   (exit column j = n: the exit
             count of row i, kept on the diagonal of the N block),
    zsum_k = sum of z_i / c over its cells in REVERSE walk order,
    theta_k ~ Gamma(nu_k + Nsum_k, scale 1 / (zeta_k + zsum_k)),

a cell's value is theta_k c, and the diagonal of row i is minus the sum of the
row's cells: by increasing column for iteration 0, by decreasing column after
every update.  The division by c is the reference's quirk: the law asserted
here is the reference's, not the model's.
"""
import functools

import numpy as np

from phasetype_amd.synth import simulate_ph

MHRS, ECS, DCS, UNIF = 1, 2, 4, 8
SAMPLER_NAMES = {MHRS: "MHRS", ECS: "ECS", DCS: "DCS", UNIF: "UNIF"}


# ------------------------------------------------------- the numpy statement
def cells(T, C):
    """[(i, j, k, c)] of the used cells in walk order"""
    T = np.asarray(T)
    C = np.asarray(C, np.float64)
    n1 = T.shape[0]
    return [(i, j, int(T[i, j]) - 1, float(C[i, j])) for i in range(n1) for j in range(n1) if T[i, j] != 0]


def update_args(T, C, nu, zeta, zq, N, zexp):
    """(shape[m], scale[m]) of the Gamma draws of one update from a sweep's
    statistics: zq[n] the fixed-point sojourn totals (z = zq 2^-zexp), N[n, n]
    the transition counts N[from, to] with the exit counts on the diagonal"""
    n = np.asarray(T).shape[0] - 1
    m = len(nu)
    z = [float(np.ldexp(np.float64(int(q)), -int(zexp))) for q in np.asarray(zq).reshape(-1)[:n]]
    N = np.asarray(N)
    Nsum = [0] * m
    zsum = [0.0] * m
    walk = cells(T, C)
    for i, j, k, c in walk:
        Nsum[k] += int(N[i, i] if j == n else N[i, j])
    for i, j, k, c in reversed(walk):
        zsum[k] = zsum[k] + z[i] / c
    shape = np.array([float(nu[k]) + float(Nsum[k]) for k in range(m)])
    scale = np.array([1.0 / (float(zeta[k]) + zsum[k]) for k in range(m)])
    return shape, scale


def assemble(theta, T, C, first):
    """(S[n, n], s[n]) of a draw: cells theta_k c; the diagonal minus the sum
    of the row's cells, by increasing column (first: iteration 0) or by
    decreasing column (after an update), one subtraction at a time"""
    T = np.asarray(T)
    n = T.shape[0] - 1
    TT = np.zeros((n + 1, n + 1))
    for i, j, k, c in cells(T, C):
        TT[i, j] = float(theta[k]) * c
    for i in range(n):
        d = 0.0
        for j in (range(n + 1) if first else range(n, -1, -1)):
            if T[i, j] != 0:
                d = d - TT[i, j]
        TT[i, i] = d
    return TT[:n, :n].copy(), TT[:n, n].copy()


# ------------------------------------------------------------ the structures
class Case:
    """A structure: T, C ((n+1)^2), priors nu, zeta, the parameter ``truth``
    its data are simulated from, and the samplers it admits."""

    def __init__(self, name, T, C, nu, zeta, truth, samplers, exact_only=()):
        self.name, self.T, self.C = name, np.asarray(T, np.int32), np.asarray(C, np.float64)
        self.nu, self.zeta = np.asarray(nu, np.float64), np.asarray(zeta, np.float64)
        self.truth, self.samplers, self.exact_only = np.asarray(truth, np.float64), tuple(samplers), tuple(exact_only)
        self.n, self.m = self.T.shape[0] - 1, len(self.nu)

    def generator(self, theta=None):
        return assemble(self.truth if theta is None else theta, self.T, self.C, True)

    def data(self, N, censor_frac=0.0, seed=None):
        S, s = self.generator()
        seed = (0x7D47E + sum(map(ord, self.name))) if seed is None else seed
        return simulate_ph(S, s, N, seed=seed, censor_frac=censor_frac)

    def tight_priors(self, y):
        """(nu, zeta) with the mode on ``truth`` and about eight times the
        data's weight: zeta_k = 8 sum(y) sum over k's cells of 1 / c bounds
        zsum_k of exact data from above eight times over.  The division by c
        moves the chain's stationary region away from the parameter the data
        came from (by c^2 on erlang3c); under weak priors the chain then sits
        where MHRS rejects nearly every path and UNIF's table overflows.  zeta
        + zsum then rounds away the last three or four bits of zsum, which
        are those a changed summation order moves: these chains pin the
        cells, counts and multipliers, and the order is pinned under the
        cases' own priors (test_gpu_update.py: the resident chains and the
        resident step on fr3c and bd10t).  A parameter without cells keeps
        its prior."""
        nu, zeta = self.nu.copy(), self.zeta.copy()
        w = np.zeros(self.m)
        for i, j, k, c in cells(self.T, self.C):
            w[k] += 1.0 / c
        used = w > 0
        zeta[used] = 8.0 * float(np.sum(y)) * w[used]
        nu[used] = 1.0 + zeta[used] * self.truth[used]
        return nu, zeta

    def censor_frac(self, method, frac=0.3):
        """DCS takes censored observations as exact: it is run on exact data"""
        return 0.0 if method == DCS or method in self.exact_only else frac


def _fill(n, entries):
    T = np.zeros((n + 1, n + 1), np.int32)
    C = np.ones((n + 1, n + 1))
    for i, j, t, c in entries:
        T[i, j], C[i, j] = t, c
    return T, C


def _fr3(scaled):
    c02, c20, c13 = (2.5, 0.75, 1.6) if scaled else (1.0, 1.0, 1.0)
    return _fill(3, [(0, 1, 1, 1.0), (0, 2, 1, c02), (1, 3, 1, c13), (2, 3, 1, 1.0), (1, 0, 2, 1.0), (2, 0, 2, c20)])


def _bd10t():
    n = 10
    ent = []
    for i in range(n):
        if i + 1 < n:
            ent.append((i, i + 1, 1, 1.0 + 0.05 * i))
        if i > 0:
            ent.append((i, i - 1, 2, 1.0))
        ent.append((i, n, 3, 0.1 * (i + 1)))
    return _fill(n, ent)


def _erlang3(c):
    return _fill(3, [(0, 1, 1, c), (1, 2, 1, c), (2, 3, 1, c)])


def _full9(scaled):
    n = 9
    rng = np.random.default_rng(0xF9)
    ent, k = [], 0
    for i in range(n):
        for j in range(n + 1):
            if i != j:
                k += 1
                ent.append((i, j, k, float(rng.uniform(0.5, 2.0)) if scaled else 1.0))
    T, C = _fill(n, ent)
    truth = np.where(np.array([e[1] for e in ent]) == n, rng.uniform(0.2, 0.6, k), rng.uniform(0.1, 0.5, k))
    return T, C, truth


def _cases():
    out = {}
    fr_nu, fr_zeta, fr_truth = (24.0, 180.0), (16.0, 16.0), (1.5, 11.25)  # the reference script's priors
    for name, scaled in (("fr3", False), ("fr3c", True)):
        T, C = _fr3(scaled)
        out[name] = Case(name, T, C, fr_nu, fr_zeta, fr_truth, (ECS, DCS, UNIF, MHRS))
    T, C = _bd10t()
    out["bd10t"] = Case("bd10t", T, C, (41.0, 11.0, 21.0), (20.0, 20.0, 20.0), (2.0, 0.5, 1.0), (ECS, DCS, UNIF, MHRS))
    for name, c in (("erlang3", 1.0), ("erlang3c", 1.7)):
        T, C = _erlang3(c)
        out[name] = Case(name, T, C, (3.0,), (2.0,), (1.3 / c,), (UNIF, MHRS))  # defective for ECS / DCS
    for name, c in (("exp1", 1.0), ("exp1c", 0.4)):
        T, C = _fill(1, [(0, 1, 1, c)])
        out[name] = Case(name, T, C, (2.5,), (1.5,), (0.8 / c,), (ECS, DCS, UNIF, MHRS))
    for name, scaled in (("full9", False), ("full9c", True)):
        T, C, truth = _full9(scaled)
        out[name] = Case(name, T, C, 1.0 + 10.0 * truth, np.full(len(truth), 10.0), truth, (UNIF, MHRS))
    T, C = _fr3(False)
    for name, nu2 in (("unused", 3.0), ("unused07", 0.7)):  # parameter 2 occurs in no cell
        out[name] = Case(name, T, C, fr_nu + (nu2,), fr_zeta + (2.0,), fr_truth + (1.0,), (ECS, UNIF))
    return out


CASES = _cases()
# every structure x admitted sampler
PAIRS = [(name, meth) for name, c in CASES.items() for meth in c.samplers]
PAIR_IDS = [f"{name}-{SAMPLER_NAMES[meth]}" for name, meth in PAIRS]


# ----------------------------------------------------- closed-form posteriors
def closed_form(name, y, cens):
    """{parameter: (shape, rate)} of the parameters whose draws are iid Gamma
    whatever the paths: erlang3(c) with exact data (every path visits the
    three states once, N = 3 per observation, and sum_i z_i = y), exp1 with
    any censoring (N = the exact observations; the draws then mix instead of
    being independent), exp1c with exact data (with censoring and c != 1 the
    chain targets no law), the unused parameter (its prior).  The rate carries the quirk: zeta + sum(y) / c."""
    c = CASES[name]
    y, cens = np.asarray(y, np.float64), np.asarray(cens)
    if name.startswith("erlang3"):
        assert not cens.any()
        return {0: (c.nu[0] + 3 * len(y), c.zeta[0] + y.sum() / c.C[0, 1])}
    if name.startswith("exp1"):
        return {0: (c.nu[0] + int((cens == 0).sum()), c.zeta[0] + y.sum() / c.C[0, 1])}
    if name.startswith("unused"):
        return {2: (c.nu[2], c.zeta[2])}
    raise KeyError(name)


def wrong_laws(name, y, cens):
    """The three wrong laws the closed-form check must reject, as {label:
    {parameter: (shape, rate)}}: one N cell dropped, sum(y) c for sum(y) / c
    (None where c = 1), the rate off by 0.5 %; all None for the unused
    parameter, whose law no statistic enters."""
    c = CASES[name]
    (k, (a, b)), = closed_form(name, y, cens).items()
    if name.startswith("unused"):  # a prior draw: no statistic enters it, and 0.5 % is not resolvable at its shape
        return {"rate_off": None, "cell_dropped": None, "times_c": None}
    out = {"rate_off": {k: (a, b * 1.005)}}
    y, cens = np.asarray(y, np.float64), np.asarray(cens)
    per_cell = len(y) if name.startswith("erlang3") else int((cens == 0).sum())
    out["cell_dropped"] = {k: (a - per_cell, b)}  # a used cell's count never reaches Nsum
    cc = float(c.C[0, 1])
    out["times_c"] = None if cc == 1.0 else {k: (a, c.zeta[0] + y.sum() * cc)}
    return out


def ks_pvalue(draws, shape, rate):
    from scipy import stats

    return float(stats.kstest(np.asarray(draws), stats.gamma(shape, scale=1.0 / rate).cdf).pvalue)


LAW_DRAWS = 20000
# observations of the closed-form cases: the 0.5 % teeth need a shape nu + Nsum of 450 or more (a shift of
# 0.005 sqrt(shape) = 0.1 standard deviations moves the CDF by 0.04, which 20,000 draws put at p ~ 1e-20)
LAW_N = {"erlang3": 150, "erlang3c": 150, "exp1": 700, "exp1c": 700, "unused": 20, "unused07": 20}
LAW_CASES = [("erlang3", UNIF), ("erlang3c", UNIF), ("exp1", ECS), ("exp1c", ECS),
             ("unused", ECS), ("unused07", UNIF)]


def law_data(name):
    c = CASES[name]
    # exp1c on exact data: with c < 1 and censored observations the update's z / c has no stationary law.  A
    # censored path runs on for Exp(theta c) past y, so zsum grows as theta falls, and with c = 0.4 the next
    # theta c is below 0.37 of the last at every sweep: the chain runs to zero and the paths without bound
    return c.data(LAW_N[name], 0.3 if name == "exp1" else 0.0)


def check_laws(name, chain, y, cen):
    """the KS bar against the closed form and the three wrong laws; returns
    the p-values for the record"""
    out = {}
    for k, (a, b) in closed_form(name, y, cen).items():
        x = chain[1:, k]
        r1 = np.corrcoef(x[:-1], x[1:])[0, 1]
        out["p"] = ks_pvalue(x, a, b)
        print(f"{name}: KS p = {out['p']:.3g}, lag-1 autocorrelation {r1:+.4f}")
        assert out["p"] > 1e-4, out
        if not cen.any():  # iid draws (censored observations are augmented: the chain mixes, its law is the same)
            assert abs(r1) < 5.0 / np.sqrt(len(x)), r1
        for label, law in wrong_laws(name, y, cen).items():
            if law is None:
                continue
            out[label] = ks_pvalue(x, *law[k])
            print(f"{name}: wrong law {label}: p = {out[label]:.3g}")
            assert out[label] < 1e-10, (label, out)
    return out


# ------------------------------------------- the fr3 posterior by quadrature
FR3_TRUTH_TOL = 1e-5  # the refinement stops when no returned value moved by more


def fr3_loglik(F, R, y, cens):
    """log-likelihood of fr3 (C = 1) at arrays F, R (one shape) from numpy's
    eigendecomposition: density pi exp(S y) s, survival pi exp(S y) 1, pi = e_1"""
    F, R = np.broadcast_arrays(np.asarray(F, np.float64), np.asarray(R, np.float64))
    shp = F.shape
    F, R = F.reshape(-1), R.reshape(-1)
    S = np.zeros((len(F), 3, 3))
    S[:, 0, 0], S[:, 0, 1], S[:, 0, 2] = -2.0 * F, F, F
    S[:, 1, 0], S[:, 1, 1] = R, -(R + F)
    S[:, 2, 0], S[:, 2, 2] = R, -(R + F)
    lam, Q = np.linalg.eig(S)
    Qi = np.linalg.inv(Q)
    assert np.abs(np.imag(lam)).max() == 0.0  # the spectrum is real: the lumped chain is a birth-death one
    lam, Q, Qi = np.real(lam), np.real(Q), np.real(Qi)
    s = np.stack([np.zeros_like(F), F, F], 1)
    a = Q[:, 0, :] * np.einsum("gkj,gj->gk", Qi, s)           # density coefficients
    b = Q[:, 0, :] * Qi.sum(2)                                 # survival coefficients
    y, cens = np.asarray(y, np.float64), np.asarray(cens)
    out = np.zeros(len(F))
    for coef, ys in ((a, y[cens == 0]), (b, y[cens != 0])):
        for lo in range(0, len(ys), 32):
            yy = ys[lo:lo + 32]
            v = np.einsum("gk,gky->gy", coef, np.exp(lam[:, :, None] * yy[None, None, :]))
            out += np.log(v).sum(1)
    return out.reshape(shp)


def _fr3_grid(y, cens, nu, zeta, G, lo, hi):
    """marginal summaries on a G x G grid, uniform in (log F, log R) over the
    box [lo, hi] (log coordinates)"""
    from scipy.interpolate import CubicSpline
    from scipy.optimize import brentq

    u = [np.linspace(lo[d], hi[d], G) for d in range(2)]
    U, V = np.meshgrid(u[0], u[1], indexing="ij")
    F, R = np.exp(U), np.exp(V)
    lp = fr3_loglik(F, R, y, cens)
    lp += (nu[0] - 1.0) * U - zeta[0] * F + (nu[1] - 1.0) * V - zeta[1] * R
    lp += U + V  # the Jacobian of the log coordinates
    w = np.exp(lp - lp.max())
    total = w.sum()
    inner = w[1:-1, 1:-1].sum()
    out = {"edge_mass": float((total - inner) / total), "G": G, "mean": np.zeros(2)}
    for q in (5, 50, 95):
        out[f"q{q:02d}"] = np.zeros(2)
    for d in range(2):
        marg = w.sum(1 - d)
        marg = marg / marg.sum()
        # a smooth density that vanishes at both ends: the equal-weight sum is
        # the trapezoid rule at its spectral accuracy
        out["mean"][d] = float((marg * np.exp(u[d])).sum())
        A = CubicSpline(u[d], marg).antiderivative()
        tot = float(A(u[d][-1]))
        for q in (5, 50, 95):
            out[f"q{q:02d}"][d] = float(np.exp(brentq(lambda x: float(A(x)) - q / 100.0 * tot, u[d][0], u[d][-1],
                                                        xtol=1e-14, rtol=1e-14)))
    return out


@functools.lru_cache(maxsize=None)
def _fr3_posterior(ykey, ckey):
    y, cens = np.frombuffer(ykey, np.float64), np.frombuffer(ckey, np.int32)
    c = CASES["fr3"]
    # the box: a coarse pass over a wide one finds the mode and the spread
    lo, hi = np.log([0.05, 0.5]), np.log([30.0, 300.0])
    for _ in range(3):
        u = [np.linspace(lo[d], hi[d], 81) for d in range(2)]
        U, V = np.meshgrid(u[0], u[1], indexing="ij")
        lp = (fr3_loglik(np.exp(U), np.exp(V), y, cens) + c.nu[0] * U - c.zeta[0] * np.exp(U)
              + c.nu[1] * V - c.zeta[1] * np.exp(V))
        w = np.exp(lp - lp.max())
        w /= w.sum()
        mu = [float((w.sum(1 - d) * u[d]).sum()) for d in range(2)]
        sd = [max(float(np.sqrt((w.sum(1 - d) * (u[d] - mu[d]) ** 2).sum())), (hi[d] - lo[d]) / 80.0) for d in range(2)]
        lo, hi = np.array([mu[d] - 9.0 * sd[d] for d in range(2)]), np.array([mu[d] + 9.0 * sd[d] for d in range(2)])
    G, prev = 160, None
    while True:
        cur = _fr3_grid(y, cens, c.nu, c.zeta, G, lo, hi)
        if prev is not None:
            move = max(float(np.abs(cur[k] - prev[k]).max()) for k in ("mean", "q05", "q50", "q95"))
            if move <= FR3_TRUTH_TOL:
                cur["last_move"] = move
                break
            assert G < 1000, ("the quadrature does not settle", G, move)
        prev, G = cur, G + G // 2
    assert cur["edge_mass"] < 1e-12, cur["edge_mass"]
    cur["box"] = (np.exp(lo), np.exp(hi))
    for k in ("mean", "q05", "q50", "q95"):
        cur[k + "_se"] = np.zeros(2)  # no Monte Carlo error
    return cur


def fr3_posterior(y, cens):
    """The exact posterior of fr3 (C = 1, the script's priors) given (y, cens):
    per parameter (F, R) the mean and the 5 / 50 / 95 % quantiles, in the
    layout of oracle.posterior.summarize with zero standard errors.  The grid
    is refined (x 1.5 a side) until no value moves by more than FR3_TRUTH_TOL
    (``last_move``: what the last refinement moved; ``G``: the final side);
    the mass of its outermost ring is below 1e-12."""
    return _fr3_posterior(np.ascontiguousarray(y, np.float64).tobytes(),
                          np.ascontiguousarray(cens, np.int32).tobytes())


def fr3_anchor(y, cens, points):
    """max |numpy - mpmath| of the log-likelihood at (F, R) ``points``: the
    anchor of the quadrature's likelihood to evaluator_cases.truth"""
    import evaluator_cases as EC

    c = CASES["fr3"]
    worst = 0.0
    for F, R in points:
        S, s = assemble((F, R), c.T, c.C, True)
        want = sum(EC.truths(S, s, y, cens))
        worst = max(worst, abs(float(fr3_loglik(F, R, y, cens)) - float(want)))
    return worst


FR3_N, FR3_SWEEPS = 150, 12001


def fr3_data(censored):
    return CASES["fr3"].data(FR3_N, 0.3 if censored else 0.0, seed=0xF3D + int(censored))


def worst_z(summ, truth):
    """max over statistics and parameters of |chain - truth| / the chain's MCSE"""
    worst = 0.0
    for st in ("mean", "q05", "q50", "q95"):
        worst = max(worst, float((np.abs(summ[st][:2] - truth[st]) / (summ[st + "_se"][:2] + 1e-300)).max()))
    return worst


def check_posterior(summ, y, cens, k_sigma, label=""):
    """A chain's summary (oracle.posterior.summarize of its F and R columns)
    within k_sigma of its own MCSEs of the exact posterior, and the teeth:
    against the posterior of 1.05 y it must miss by more than 8"""
    truth = fr3_posterior(y, cens)
    mcse = min(float(summ[k + "_se"][:2].min()) for k in ("mean", "q05", "q50", "q95"))
    assert truth["last_move"] <= 0.1 * mcse, (truth["last_move"], mcse)
    z = worst_z(summ, truth)
    z105 = worst_z(summ, fr3_posterior(1.05 * np.asarray(y), cens))
    print(f"{label}: worst |z| = {z:.2f}; against 1.05 y: {z105:.2f}")
    assert z <= k_sigma, (z, summ, truth)
    assert z105 > 8.0, z105
    return z, z105


# ------------------------------- literals of tests/host/host_lists_check.cpp
def host_check_cases():
    """The two hand-written runs the stand-alone GibbsState check replays:
    (name, T, C, nu, zeta, start or None, preset draws, [(zq, N)] per update,
    zexp).  tri3 has three cells per parameter; its row 0 sums differently by
    increasing and by decreasing column."""
    T, C = _fr3(True)
    fr = ("fr3c", T, C, (24.0, 180.0), (16.0, 16.0), (1.5, 11.25), (1.375, 10.5, 1.625, 12.25),
          [((517, 1283, 2051), [[0, 7, 5], [6, 4, 0], [3, 0, 8]]), ((333, 777, 1111), [[0, 2, 9], [1, 11, 0], [13, 0, 3]])],
          10)
    T, C = _fill(3, [(0, 1, 1, 2.0 ** 53), (0, 2, 1, 1.0), (0, 3, 1, 1.0), (1, 3, 2, 0.5), (2, 0, 2, 3.0), (2, 3, 2, 1.25)])
    tri = ("tri3", T, C, (2.0, 0.7), (4.0, 2.0), None, (0.3, 0.75, 1.7, 1.0, 0.9),
           [((1001, 2003, 3007), [[5, 3, 2], [0, 9, 0], [4, 0, 6]]), ((4099, 123, 2999), [[1, 8, 7], [0, 2, 0], [10, 0, 12]])],
           11)
    return [fr, tri]


def host_check_literals():
    """The C++ literals (hex floats) of host_lists_check.cpp's GibbsState runs"""
    def arr(name, v):
        return f"  static const double {name}[] = {{{', '.join(float(x).hex() for x in np.asarray(v).reshape(-1, order='F'))}}};"

    def full(S, s):
        n = len(s)
        TT = np.zeros((n + 1, n + 1))
        TT[:n, :n], TT[:n, n] = S, s
        return TT

    out = []
    for name, T, C, nu, zeta, start, preset, stats, zexp in host_check_cases():
        draws = list(preset)
        theta = list(start) if start is not None else [(nu[k] - 1.0) / zeta[k] if nu[k] > 1 else draws.pop(0)
                                                        for k in range(len(nu))]
        S, s = assemble(theta, T, C, True)
        Sr, sr = assemble(theta, T, C, False)
        if name == "tri3":
            assert S[0, 0] != Sr[0, 0]  # the two orders differ on row 0
        out += [f"  /* {name}: constructor */", arr(f"{name}_TT0", full(S, s))]
        for u, (zq, N) in enumerate(stats, 1):
            shape, scale = update_args(T, C, nu, zeta, zq, N, zexp)
            theta = [draws.pop(0) for _ in nu]
            S, s = assemble(theta, T, C, False)
            out += [f"  /* {name}: update {u} */", arr(f"{name}_args{u}", np.stack([shape, scale], 1).T),
                    arr(f"{name}_TT{u}", full(S, s))]
    return "\n".join(out)


if __name__ == "__main__":
    print(host_check_literals())
