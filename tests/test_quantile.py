"""CPU: the quantile specification (include/pht_quantile.h) through the tests'
restatement (tests/quantile_spec.c) and the host-only library function; no GPU.

* Certificate: every finite root's bracket has h(lo) >= 0 >= h(hi), recomputed
  with the uniformisation restatement, and satisfies the stop rule.
* Truth: mpmath at 50 digits, |log Fbar_true - L| within the header's bound at
  both ends of the bracket (so at t^ between them); the observed fraction of
  the bound is printed (recorded in DESIGN.md 5h).
* Closed forms (n = 1, Erlang), held to the bound translated to t through the
  hazard.
* Properties: monotone in p, the residual-life identity, the caller's order.
* Edge values and flags; the iteration cap is never reached.
* pht_quantile_host through the library equals the restatement bit for bit.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import evaluator_cases as EC  # noqa: E402
import loglik_unif_ref as U  # noqa: E402
import quantile_ref as Q  # noqa: E402
import phasetype_amd as P  # noqa: E402
from phasetype_amd.synth import bd_exit  # noqa: E402


def _ring10_zeros():
    S, s = U.ring(10)
    s = s.copy()
    s[:3] = 0.0  # structural zeros: no density at 0
    for i in range(10):
        S[i, i] = -(S[i].sum() - S[i, i] + s[i])
    return S, s


CASES = {
    "bd3": lambda: bd_exit(3),
    "bd10": lambda: bd_exit(10),
    "bd20": lambda: bd_exit(20),
    "CYCLIC": lambda: U.CYCLIC,
    "ring5": lambda: U.ring(5),
    "ring10_s123_zero": _ring10_zeros,
    "n1": lambda: (np.array([[-0.7]]), np.array([0.7])),
    # off BD-exit (tests/evaluator_cases.py): real spectra that are defective or nearly defective (the
    # stiff family is not here: its median lies beyond the horizon, PHT_Q_F_BEYOND, as documented)
    "erlang6": lambda: EC.erlang(6),
    "coxian_shared6": lambda: EC.coxian_shared(6),
    "gapped6": lambda: EC.gapped(6, eps=1e-9),
    "hypoexp6": lambda: EC.hypoexp(6),
    "neareq6": lambda: EC.generator("neareq", 6),
}
PROBS = np.array([1e-6, 1e-3, 0.1, 0.5, 0.9, 1 - 1e-9])
_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _mean_life(S):
    return float(np.linalg.solve(-np.asarray(S), np.ones(len(S)))[0])


def _case(name, cond):
    """the generator, t0 (0, or one mean life) and the restatement's roots at
    PROBS, computed once"""
    if (name, cond) not in _CACHE:
        S, s = CASES[name]()
        t0 = _mean_life(S) if cond else 0.0
        _CACHE[(name, cond)] = (S, s, t0, Q.quantile([S], [s], PROBS, given=t0))
    return _CACHE[(name, cond)]


ALL = [(name, cond) for name in CASES for cond in (0, 1)]


@pytest.mark.parametrize("name,cond", ALL)
def test_certificate(name, cond):
    S, s, t0, r = _case(name, cond)
    assert not r["bad_draw"][0] and not r["flags"].any(), r["flags"]
    lo, hi = r["lo"][0], r["hi"][0]
    L = Q.target(S, s, PROBS, t0)
    la, lb = Q.logsurv(S, s, lo)[0], Q.logsurv(S, s, hi)[0]
    assert np.all(la - L >= 0) and np.all(lb - L <= 0), (la - L, lb - L)
    assert np.all(lo >= t0) and np.all(lo <= hi) and np.all(hi <= Q.meta(S, s)["thi"])
    assert np.all(Q.stop_holds(lo, hi))
    that = r["t"][0] + t0 if t0 > 0 else r["t"][0]
    assert np.all(that >= lo * (1 - 2.0 ** -52)) and np.all(that <= hi * (1 + 2.0 ** -52))
    print(f"{name} t0 {t0:.4g}: evaluations {r['nev'][0].tolist()}")


@pytest.mark.parametrize("name,cond", ALL)
def test_restatement_against_mpmath(name, cond):
    import mpmath as mp

    S, s, t0, r = _case(name, cond)
    lo, hi = r["lo"][0], r["hi"][0]
    assert np.all(np.isfinite(r["t"][0])), "every root of the truth test lies within the horizon"
    b = Q.bound(S, s, PROBS, lo, hi, given=t0)
    with mp.workdps(50):
        l0 = Q.mp_logsurv(S, [t0])[0] if t0 > 0 else mp.mpf(0)
        Lt = [mp.log(1 - mp.mpf(float(p))) + l0 for p in PROBS]
        # the true roots lie within the horizon too: Fbar_true(t_hi) < 1 - p
        assert Q.mp_logsurv(S, [Q.meta(S, s)["thi"]])[0] < min(Lt)
        ea = [abs(float(v - L)) for v, L in zip(Q.mp_logsurv(S, lo), Lt)]
        eb = [abs(float(v - L)) for v, L in zip(Q.mp_logsurv(S, hi), Lt)]
    err = np.maximum(ea, eb)
    print(f"{name} t0 {t0:.4g}: max error {err.max():.3e}, bound there {b[np.argmax(err / b)]:.3e}, "
          f"largest fraction {np.max(err / b):.4f}")
    assert np.all(err <= b), (name, err, b)


def test_closed_form_exponential():
    S, s = CASES["n1"]()
    for t0 in (0.0, 1.3):
        r = Q.quantile([S], [s], PROBS, given=t0)
        want = -np.log1p(-PROBS) / s[0]  # memoryless: the residual life has the same law
        tol = Q.bound(S, s, PROBS, r["lo"][0], r["hi"][0], given=t0) / s[0] + 4 * 2.0 ** -53 * want
        if t0 > 0:
            tol = tol + 2.0 ** -53 * (t0 + want)  # t^ - t0 rounds once more
        assert np.all(np.abs(r["t"][0] - want) <= tol), (r["t"][0] - want, tol)


def test_closed_form_erlang():
    from scipy.stats import gamma

    k, rate = 4, 1.5
    S = np.diag(np.full(k, -rate)) + np.diag(np.full(k - 1, rate), 1)
    s = np.zeros(k)
    s[-1] = rate
    p = np.array([1e-3, 0.1, 0.5, 0.9, 1 - 1e-6])
    r = Q.quantile([S], [s], p)
    assert not r["flags"].any()
    want = gamma.ppf(p, k, scale=1 / rate)
    hz = gamma.pdf(want, k, scale=1 / rate) / gamma.sf(want, k, scale=1 / rate)
    # the reference's own residual, translated to t, and 8 ulp of its value
    ref_err = np.abs(gamma.sf(want, k, scale=1 / rate) - (1 - p)) / gamma.pdf(want, k, scale=1 / rate) \
        + 8 * 2.0 ** -53 * want
    tol = Q.bound(S, s, p, r["lo"][0], r["hi"][0]) / hz + ref_err
    print("erlang: error / tolerance", np.abs(r["t"][0] - want) / tol)
    assert np.all(np.abs(r["t"][0] - want) <= tol), (r["t"][0] - want, tol)


def test_monotone_in_p_and_callers_order():
    S, s = bd_exit(10)
    p = np.arange(1, 100) / 100.0
    for t0 in (0.0, 2.0):
        r = Q.quantile([S], [s], p, given=t0)
        assert not r["flags"].any() and np.all(np.diff(r["t"][0]) >= 0)
        # unsorted, with duplicates: each root is its probability's
        rng = np.random.default_rng(5)
        idx = rng.integers(0, len(p), 150)
        g = P.quantile_host(S, s, p[idx], given=t0)
        for k in ("t", "lo", "hi"):
            assert np.array_equal(_bits(g[k]), _bits(r[k][0][idx])), k
        assert np.array_equal(g["nev"], r["nev"][0][idx])


@pytest.mark.parametrize("name", ["bd10", "CYCLIC", "ring10_s123_zero"])
def test_residual_life_identity(name):
    """t0 + q(p | t0) against q(1 - (1 - p) Fbar(t0)), within the two bounds
    translated to t through the hazard there"""
    import mpmath as mp

    S, s, t0, r = _case(name, 1)
    p = PROBS[1:5]
    with mp.workdps(50):
        F0 = mp.exp(Q.mp_logsurv(S, [t0])[0])
        p2 = np.array([float(1 - (1 - mp.mpf(float(v))) * F0) for v in p])
    u = Q.quantile([S], [s], p2)
    assert not u["flags"].any()
    lhs, rhs = t0 + r["t"][0][1:5], u["t"][0]
    hz = Q.hazard(S, s, rhs)
    b1 = Q.bound(S, s, p, r["lo"][0][1:5], r["hi"][0][1:5], given=t0)
    b2 = Q.bound(S, s, p2, u["lo"][0], u["hi"][0])
    # p2 is rounded to a double once: log(1 - p2) moves by 2^-53 p2 / (1 - p2)
    tol = (b1 + b2 + 2.0 ** -53 * p2 / (1 - p2)) / hz + 2 * 2.0 ** -53 * rhs
    assert np.all(np.abs(lhs - rhs) <= tol), (lhs - rhs, tol)


def test_edge_values_and_flags():
    S, s = bd_exit(3)
    pr = np.array([0.0, 1.0, np.nan, -0.1, 1.5, 0.5])
    for t0 in (0.0, 0.75):
        r = Q.quantile([S], [s], pr, given=t0)
        t, f = r["t"][0], r["flags"][0]
        assert t[0] == 0.0 and r["lo"][0][0] == t0 and r["hi"][0][0] == t0 and f[0] == 0
        assert t[1] == np.inf and f[1] == 0
        assert np.all(np.isnan(t[2:5])) and np.all(f[2:5] == Q.F_P)
        assert np.isfinite(t[5]) and f[5] == 0
        assert np.all(r["nev"][0][:5] == 0)
    r = Q.quantile([S], [s], pr, given=-1.0)
    assert np.all(np.isnan(r["t"][0][[0, 1, 5]])) and np.all(r["flags"][0][[0, 1, 5]] == Q.F_T0)
    r = Q.quantile([S], [s], [0.5], given=np.inf)
    assert np.isnan(r["t"][0][0]) and r["flags"][0][0] == Q.F_T0


def test_flagged_draw_is_never_evaluated():
    S, s = bd_exit(3)
    Sn = S.copy()
    Sn[1, 1] = np.nan
    r = Q.quantile([S, Sn, S], [s, s, s], [0.0, 0.5, 1.0])
    assert r["bad_draw"].tolist() == [False, True, False] and r["draw_flags"][1] == P.LL_F_NONFINITE
    assert np.all(np.isnan(r["t"][1])) and np.all(r["flags"][1] == Q.F_DRAW) and np.all(r["nev"][1] == 0)
    assert np.array_equal(_bits(r["t"][0]), _bits(r["t"][2]))
    z = Q.quantile([np.zeros((2, 2))], [np.zeros(2)], [0.5])  # no positive rate
    assert z["bad_draw"][0] and z["flags"][0][0] == Q.F_DRAW


def test_beyond_the_horizon():
    S, s = bd_exit(3)
    full = Q.quantile([S], [s], [0.1, 0.9])["t"][0]
    r = Q.quantile([S], [s], [0.1, 0.9], tmax=1.0)
    assert full[0] < 1.0 < full[1]
    assert r["flags"][0].tolist() == [0, Q.F_BEYOND] and r["t"][0][1] == np.inf
    assert r["lo"][0][1] == 1.0 and r["hi"][0][1] == np.inf
    assert abs(r["t"][0][0] - full[0]) <= 2.0 ** -43 * full[0]
    # conditioning beyond the horizon
    r = Q.quantile([S], [s], [0.5], given=2.0, tmax=1.0)
    assert r["flags"][0][0] == Q.F_BEYOND and r["t"][0][0] == np.inf and r["nev"][0][0] == 0
    # a generator that never absorbs: Fbar = 1
    Sn = np.array([[-1.0, 1.0], [1.0, -1.0]])
    for t0 in (0.0, 3.0):
        r = Q.quantile([Sn], [np.zeros(2)], [1e-9, 0.5], given=t0)
        assert np.all(r["flags"][0] == Q.F_BEYOND) and np.all(r["t"][0] == np.inf), r


def test_the_cap_is_never_reached():
    worst = 0
    for key, (S, s, t0, r) in list(_CACHE.items()):
        assert not (r["flags"] & Q.F_CAP).any()
        worst = max(worst, int(r["nev"].max()))
    S, s = bd_exit(10)
    r = Q.quantile([S], [s], [1e-300, 1e-15, 1 - 2.0 ** -53], given=0.0)
    assert not (r["flags"] & Q.F_CAP).any(), r["flags"]
    worst = max(worst, int(r["nev"].max()))
    print("largest evaluation count of a root:", worst)
    assert worst < 2 * Q.spec().qspec_maxit()


def test_horizon_constant():
    L = Q.spec()
    assert L.qspec_lambda() == 1400.0 and L.qspec_rtol() == 2.0 ** -44
    for S, s in (bd_exit(3), CASES["n1"](), bd_exit(20)):
        m = Q.meta(S, s)
        assert m["K"] == 1988 and m["thi"] == 1400.0 / m["mu"]
    assert Q.meta(*bd_exit(3), tmax=2.0)["thi"] == 2.0 and Q.meta(*bd_exit(3), tmax=2.0)["K"] < 200


@pytest.mark.parametrize("name", list(CASES))
def test_library_host_function_is_the_restatement(lib, name):
    S, s = CASES[name]()
    pr = np.array([0.5, 1e-3, np.nan, 0.0, 1.0, 0.9, 0.5, -0.1, 1 - 1e-9])
    for t0, tmax in ((0.0, None), (_mean_life(S), None), (0.3, 2.0)):
        g = P.quantile_host(S, s, pr, given=t0, tmax=tmax)
        w = Q.quantile([S], [s], pr, given=t0, tmax=np.inf if tmax is None else tmax)
        for k in ("t", "lo", "hi"):
            assert np.array_equal(_bits(g[k]), _bits(w[k][0])), (name, t0, k)
        assert np.array_equal(g["nev"], w["nev"][0]) and np.array_equal(g["flags"], w["flags"][0])
        assert g["bad_draw"] == bool(w["bad_draw"][0])
    with pytest.raises(P.PhaseTypeError):
        P.quantile_host(S, s, pr, tmax=0.0)
