"""CPU: the uniformisation log-likelihood specification
(include/pht_loglik_unif.h) through the tests' restatement
(tests/loglik_unif_spec.c); no GPU.

* The restatement against mpmath.expm at 50 digits on generators with a
  complex spectrum, within the specification's a-priori bound
  2^-53 (n + 9) (k_hi + 1) + 2^-56 (no cond(Q) in it); no observation bad.
* The far tail (ring(5), y up to 200), which a Poisson-only stop rule gets
  wrong by 3e-8.
* Real spectra: agreement with the spectral restatement within the sum of the
  two evaluators' bounds.
* Every family of tests/evaluator_cases.py (real spectra off BD-exit, the
  defective and nearly defective ones included) against the truth, within the
  bound plus one ulp(l).
* Table sanity, the table cap, draw flags, the K rule.
* The run splitter of evaluator="auto", and its routing of ill-conditioned
  draws and of draws with a bad observation.
"""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import evaluator_cases as EC  # noqa: E402
import loglik_ref as R  # noqa: E402
import loglik_unif_ref as U  # noqa: E402
import phasetype_amd as P  # noqa: E402
from phasetype_amd.synth import simulate_ph  # noqa: E402


def _ring10_zeros():
    S, s = U.ring(10)
    s = s.copy()
    s[:3] = 0.0  # structural zeros: a_0 = a_1 = a_2 = 0
    for i in range(10):
        S[i, i] = -(S[i].sum() - S[i, i] + s[i])
    return S, s


CASES = {
    "CYCLIC": lambda: U.CYCLIC,
    "ring5": lambda: U.ring(5),
    "ring10": lambda: U.ring(10),
    "ring20": lambda: U.ring(20),
    "ring10_s123_zero": _ring10_zeros,
}
Y_TAIL = np.arange(20.0, 201.0, 20.0)  # ring(5) only


def _obs(name, S, s):
    y, cens = simulate_ph(S, s, 40, seed=1, censor_frac=0.3)
    y, cens = U.with_edges(y, cens)
    if name == "ring5":
        y, cens = U.with_edges(y, cens, list(Y_TAIL))
    return y, cens


def _truth(S, s, y, cens):
    import mpmath as mp

    n = S.shape[0]
    out = []
    with mp.workdps(50):
        Sm = mp.matrix(S.tolist())
        sv = mp.matrix(s.tolist())
        one = mp.matrix([1.0] * n)
        cache = {}
        for yi, ci in zip(y, cens):
            if yi not in cache:
                cache[yi] = mp.expm(Sm * mp.mpf(float(yi)))
            E = cache[yi]
            v = sv if ci == 0 else one
            out.append(mp.log(sum(E[0, j] * v[j] for j in range(n))))
    return out


def _check_against_mpmath(tag, S, s, y, cens):
    import mpmath as mp

    n = S.shape[0]
    l, khi = U.pointwise([S], [s], y, cens, with_khi=True)
    assert np.all(np.isfinite(l)), (tag, "no observation of these inputs is bad", y[~np.isfinite(l[0])])
    truth = _truth(S, s, y, cens)
    worst = 0.0
    bounds = U.bound(n, khi[0])
    for li, ti, yi, bi in zip(l[0], truth, y, bounds):
        err = float(abs(mp.mpf(float(li)) - ti))
        worst = max(worst, err / bi)
    print(f"{tag}: n={n}, worst error / bound = {worst:.3g}, largest k_hi = {int(khi.max())}")
    for li, ti, yi, bi in zip(l[0], truth, y, bounds):
        err = float(abs(mp.mpf(float(li)) - ti))
        assert err <= bi, (tag, yi, li, float(ti), err, bi)


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_against_mpmath(name):
    S, s = CASES[name]()
    assert np.any(np.abs(np.linalg.eigvals(S).imag) > 0), "these generators have a complex spectrum"
    y, cens = _obs(name, S, s)
    _check_against_mpmath(name, S, s, y, cens)


def test_far_tail_regression():
    """ring(5) at y = 50, 100, 200: the sum's mode lies far below the Poisson
    mode, and a stop rule on the Poisson weight alone ends the downward sweep
    too early (3e-8 at l = -107)."""
    S, s = U.ring(5)
    y = np.array([50.0, 100.0, 200.0, 50.0, 100.0, 200.0])
    cens = np.array([0, 0, 0, 1, 1, 1], np.int32)
    _check_against_mpmath("far tail ring5", S, s, y, cens)
    l = U.pointwise([S], [s], y, cens)[0]
    assert l[2] < -100


@pytest.mark.parametrize("n", [5, 10])
def test_real_spectra_agree_with_the_spectral_evaluator(lib, n):
    Ss, ss = R.scaled_draws(n)
    y, cens = simulate_ph(Ss[2], ss[2], 60, seed=1, censor_frac=0.3)
    y, cens = U.with_edges(y, cens)
    blocks = np.stack([P.loglik_block(a, b) for a, b in zip(Ss, ss)])
    assert not np.any(blocks[:, :8].view(np.uint64))
    spectral = R.pointwise(blocks, y, cens)
    unif, khi = U.pointwise(Ss, ss, y, cens, with_khi=True)
    assert np.all(np.isfinite(spectral)) and np.all(np.isfinite(unif))
    worst = 0.0
    for d, S in enumerate(Ss):
        cond = np.linalg.cond(np.linalg.eig(S)[1], 2)
        b = 64 * 2.0 ** -52 * cond + 1e-13 * np.abs(spectral[d]) + U.bound(n, khi[d])
        diff = np.abs(spectral[d] - unif[d])
        worst = max(worst, float(np.max(diff / b)))
        assert np.all(diff <= b), (n, d, float(np.max(diff / b)))
    print(f"n={n}: worst |spectral - unif| / (sum of bounds) = {worst:.3g}")


@pytest.mark.parametrize("case", EC.CASES, ids=EC.case_id)
def test_unif_on_real_spectra(case):
    """The restatement on every family of tests/evaluator_cases.py (real
    spectra: well conditioned, stiff, defective, nearly defective), y from
    1e-9 to 60, against the truth: within the a-priori bound plus one ulp(l),
    no observation bad.  Without the ulp(l) three pairs miss, all exact at
    y = 1e-9 on an Erlang chain with the rates 1e-12 or 1e-9 apart: n = 3
    (l = -41.35, k_hi = 2) by a factor 1.28, n = 6 and 10 by 1.01 and 1.02;
    Erlang(3) itself is at 0.91."""
    import mpmath as mp

    family, n, kw = case
    S, s = EC.generator(family, n, **kw)
    y, cens = EC.observations(S)
    l, khi = U.pointwise([S], [s], y, cens, with_khi=True)
    assert np.all(np.isfinite(l)), (EC.case_id(case), "no observation is bad", y[~np.isfinite(l[0])])
    truth = EC.truths(S, s, y, cens)
    err = np.array([float(abs(mp.mpf(float(li)) - ti)) for li, ti in zip(l[0], truth)])
    series, full = U.bound(n, khi[0]), U.bound(n, khi[0], l[0])
    k = int(np.argmax(err / series))
    print(f"{EC.case_id(case)}: worst error / (bound + ulp) = {np.max(err / full):.3g}; worst error / series bound "
          f"= {err[k] / series[k]:.3g} at y = {y[k]:g}, cens = {cens[k]}, l = {l[0][k]:.6g}, k_hi = {khi[0][k]}")
    assert np.all(err <= full), (EC.case_id(case), y[err > full], err[err > full], full[err > full])


def test_auto_routes_ill_conditioned_draws(lib):
    """evaluator="auto" on bd, Erlang, nearly equal rates, a complex spectrum,
    a non-finite generator and a well-conditioned chain with a bad observation
    (hypoexp(3) at y = 1e-9): the flagged draws and the one with nbad > 0 go
    to uniformisation, and every finite-generator draw ends within its
    evaluator's bound of the truth."""
    import mpmath as mp

    bdS, bds = EC.generator("bd", 3)
    nonfin = bdS.copy()
    nonfin[1, 0] = np.nan
    draws = [(bdS, bds), EC.erlang(3), EC.gapped(6, eps=1e-3), U.CYCLIC, (nonfin, bds), EC.hypoexp(3), (bdS, bds)]
    obs = [EC.observations(bdS if k == 4 else S) for k, (S, s) in enumerate(draws)]
    blocks = [P.loglik_block(S, s) for S, s in draws]
    flags = np.array([int(b[:8].view(np.uint64)[0]) for b in blocks], np.uint64)
    assert flags[0] == 0 and flags[1] & P.LL_F_ILLCOND and flags[2] & P.LL_F_ILLCOND
    assert flags[3] & P.LL_F_COMPLEX and flags[4] == P.LL_F_NONFINITE and flags[5] == 0
    spectral = [R.pointwise(b[None, :], y, c)[0] for b, (y, c) in zip(blocks, obs)]
    nbad = np.array([R.totals(l[None, :])[0][2] if f == 0 else 0 for l, f in zip(spectral, flags)])
    assert nbad.tolist() == [0, 0, 0, 0, 0, nbad[5], 0] and nbad[5] > 0
    # without the spectral pre-pass hypoexp(3) stays spectral (total -inf)
    assert P.evaluator_runs(flags) == [(0, 1, False), (1, 4, True), (4, 7, False)]
    runs = P.evaluator_runs(flags, nbad)
    assert runs == [(0, 1, False), (1, 4, True), (4, 5, False), (5, 6, True), (6, 7, False)]
    for lo, hi, unif in runs:
        for d in range(lo, hi):
            (S, s), (y, cens) = draws[d], obs[d]
            if d == 4:
                assert np.all(np.isnan(spectral[d]))
                assert np.all(np.isnan(U.pointwise([S], [s], y, cens)))
                continue
            truth = EC.truths(S, s, y, cens)
            if unif:
                l, khi = U.pointwise([S], [s], y, cens, with_khi=True)
                bounds = U.bound(S.shape[0], khi[0], l[0])
                l = l[0]
            else:
                l = spectral[d]
                bounds = [EC.spectral_bound(A, t) for A, t in zip(EC.spectral_A(blocks[d], y, cens), truth)]
            assert np.all(np.isfinite(l)), (d, unif)
            for li, ti, bi in zip(l, truth, bounds):
                assert float(abs(mp.mpf(float(li)) - ti)) <= bi, (d, unif, li, float(ti), bi)


@pytest.mark.parametrize("name", ["CYCLIC", "ring10", "ring20"])
def test_table_sanity(name):
    S, s = CASES[name]()
    n = S.shape[0]
    t = U.table(S, s, 30.0)
    assert t["flag"] == 0 and t["mu"] == np.max(-np.diag(S)) and t["abar"] == np.max(s)
    ax, ac = t["tab"][:, 0], t["tab"][:, 1]
    assert len(ax) == t["K"] + 1 and ax[0] == s[0] and ac[0] == 1.0
    assert np.all(ac >= 0) and np.all(ac <= 1) and np.all(ax >= 0) and np.all(ax <= np.max(s))
    assert np.all(np.diff(ac) <= 0)
    k = np.arange(t["K"])
    # survival after one more step: ac_{k+1} = ac_k - ax_k / mu
    assert np.all(np.abs(ac[1:] - (ac[:-1] - ax[:-1] / t["mu"])) <= (k + 1) * (n + 1) * 2.0 ** -52 * ac[0])


def test_observation_beyond_the_table_is_bad():
    """mu y = 2400 lies beyond the last row the cap allows: counted bad, not
    summed."""
    S, s = U.ring(5)
    y = np.array([1.0, 2.0, 600.0, 600.0])
    cens = np.array([0, 1, 0, 1], np.int32)
    t = U.table(S, s, y.max())
    assert t["K"] == 2047 and t["mu"] * 600.0 > 2047
    l = U.pointwise([S], [s], y, cens)
    assert np.all(np.isfinite(l[0, :2])) and np.all(np.isnan(l[0, 2:]))
    tot = R.totals(l)[0]
    assert tot[2] == 2 and tot[3] == 2
    assert P.loglik_total(tot[0:1], tot[1:2], tot[2:3], [False])[0] == -np.inf
    # the same two observations alone, in a context whose y_max they are
    good = U.pointwise([S], [s], y[:2], cens[:2])
    tg = R.totals(good)[0]
    assert np.array_equal(tot[[0, 1]], tg[[0, 1]])
    # a negative or NaN observation is bad as well
    assert np.all(np.isnan(U.pointwise([S], [s], np.array([-1.0, np.nan]), np.zeros(2, np.int32), ymax=5.0)))


def test_draw_flags():
    S, s = U.ring(5)
    Sn = S.copy()
    Sn[1, 0] = np.nan
    t = U.table(Sn, s, 10.0)
    assert t["flag"] == 4 and t["tab"] is None and t["K"] == 0
    sn = s.copy()
    sn[2] = np.inf
    assert U.table(S, sn, 10.0)["flag"] == 4
    assert U.table(np.zeros((3, 3)), np.ones(3), 10.0)["flag"] == P.LL_F_MU == 8
    # a flagged draw is never evaluated
    assert np.all(np.isnan(U.pointwise([Sn], [s], np.array([1.0, 2.0]), np.zeros(2, np.int32))))


def test_K_rule():
    for mu, ymax in ((1.1, 3.0), (4.5, 30.0), (4.5, 100.0), (4.5, 311.0), (4.5, 400.0), (1e-3, 1e-9), (7.0, 1e9)):
        lam = mu * ymax
        want = min(2047, math.ceil(lam + 14.0 * math.sqrt(lam) + 64.0))
        assert U.K_of(mu, ymax) == want, (mu, ymax)
    assert U.K_of(1.0, 0.0) == 64 and U.K_of(4.5, 400.0) == 2047


def test_evaluator_runs():
    F = P.LL_F_COMPLEX
    assert P.evaluator_runs([]) == []
    assert P.evaluator_runs([0, 0, 0]) == [(0, 3, False)]
    assert P.evaluator_runs([F, F]) == [(0, 2, True)]
    assert P.evaluator_runs([0, F, 0, F]) == [(0, 1, False), (1, 2, True), (2, 3, False), (3, 4, True)]
    assert P.evaluator_runs([0, 0, F, 0, F, F]) == [(0, 2, False), (2, 3, True), (3, 4, False), (4, 6, True)]
    # dgeevx failures go to uniformisation, non-finite generators nowhere (NaN from the spectral run)
    assert P.evaluator_runs([P.LL_F_INFO, F, P.LL_F_NONFINITE, F | P.LL_F_NONFINITE, 0]) == [(0, 2, True), (2, 5, False)]
    runs = P.evaluator_runs(np.array([0, F, F, 0, 0, F], np.uint64))
    assert [r[0] for r in runs] == [0, 1, 3, 5] and [r[1] for r in runs] == [1, 3, 5, 6]
    assert P.EVALUATORS == ("spectral", "unif", "auto")
    # ill-conditioned coefficients go to uniformisation like a complex spectrum; so does a usable block with a
    # bad observation once the spectral pre-pass has counted it (a flagged draw's count is not looked at)
    I = P.LL_F_ILLCOND
    assert P.evaluator_runs([0, I, F | I, I | P.LL_F_NONFINITE]) == [(0, 1, False), (1, 3, True), (3, 4, False)]
    assert P.evaluator_runs([0, 0, F, P.LL_F_NONFINITE], [0, 2, 0, 5]) == [(0, 1, False), (1, 3, True), (3, 4, False)]
    assert P.evaluator_runs([0, 0], [0, 0]) == P.evaluator_runs([0, 0]) == [(0, 2, False)]
