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
* Table sanity, the table cap, draw flags, the K rule.
* The run splitter of evaluator="auto".
"""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

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
