"""CPU: the E-step specification (include/pht_estep.h) through the tests'
restatement (tests/estep_spec.c) and the host-only library functions; no GPU.

* The restatement against mpmath at 50 digits (Van Loan block exponentials)
  within the header's a-priori bound; the observed fraction of the bound is
  printed (recorded in DESIGN.md 5g).
* Invariants: sum_k G per class, sum_i Z_i = sum y, sum_i E_i = exact
  observations, sum_i A_i = censored ones, totals bit-equal to the
  uniformisation evaluator's.
* The score identity (Fisher): central differences of the uniformisation
  restatement's log-likelihood against N / rate - Z.
* Sharding: integer words add exactly; pht_estep_contract through the library
  equals the restatement bit for bit.
* ph_em driven by the restatement: monotone log-likelihood, tied parameters,
  C != 1 (where a z / C M-step is not monotone), MAP.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import estep_ref as R  # noqa: E402
import evaluator_cases as EC  # noqa: E402
import loglik_unif_ref as U  # noqa: E402
import phasetype_amd as P  # noqa: E402
from phasetype_amd.synth import bd_exit, simulate_ph  # noqa: E402


def _ring10_zeros():
    S, s = U.ring(10)
    s = s.copy()
    s[:3] = 0.0  # structural zeros: a_0 = a_1 = a_2 = 0
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
}
_CACHE = {}


def _case(name):
    """the generator, ~30 simulated observations plus the edge y's (each exact
    and censored) and the restatement's E-step, computed once"""
    if name not in _CACHE:
        S, s = CASES[name]()
        y, cens = simulate_ph(S, s, 30, seed=2, censor_frac=0.3)
        y, cens = U.with_edges(y, cens)
        _CACHE[name] = (S, s, y, cens, R.estep(S, s, y, cens))
    return _CACHE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_against_mpmath(name):
    S, s, y, cens, r = _case(name)
    n = S.shape[0]
    assert r["flag"] == 0 and r["nbad"] == 0
    m = R.mp_reference(S, s, y, cens)
    good = np.ones(len(y), bool)
    b = R.bounds(n, y, cens, r["klo"], r["khi"], good, r["yscale"])
    for k in "ZNEA":
        err = float(np.max(np.abs(r[k] - m[k])))
        print(f"{name} {k}: max error {err:.3e}, bound {b[k]:.3e}, fraction {err / b[k]:.4f}")
        assert err <= b[k], (name, k, err, b[k])
    # the window's l is the evaluator's, and both are the truth's
    assert np.max(np.abs(r["l"] - m["l"])) <= np.max(U.bound(n, r["khi"]))


# off BD-exit (tests/evaluator_cases.py): one generator per family whose real
# spectrum is defective, nearly defective or stiff, on its grid of y from 1e-9
# to 60, each exact and censored
OFF_BD = {
    "erlang3": lambda: EC.erlang(3),
    "coxian_shared6": lambda: EC.coxian_shared(6),
    "gapped3": lambda: EC.gapped(3, eps=1e-9),
    "hypoexp6": lambda: EC.hypoexp(6),
    "stiff6": lambda: EC.stiff(6),
}


@pytest.mark.parametrize("name", list(OFF_BD))
def test_restatement_against_mpmath_off_bd_exit(name):
    """The same check on the series the evaluators share, where the spectral
    evaluator gives up.  The truth's digits grow with n and -log10 y: an entry
    of the block exponential is as small as y^(2 n - 1) and expm's error is
    absolute."""
    S, s = OFF_BD[name]()
    n = S.shape[0]
    y, cens = EC.observations(S)
    r = R.estep(S, s, y, cens)
    assert r["flag"] == 0 and r["nbad"] == 0
    m = R.mp_reference(S, s, y, cens, dps=60 + 6 * n * 9 + int(np.max(-np.diag(S)) * y.max() / np.log(10.0)))
    b = R.bounds(n, y, cens, r["klo"], r["khi"], np.ones(len(y), bool), r["yscale"])
    for k in "ZNEA":
        err = float(np.max(np.abs(r[k] - m[k])))
        print(f"{name} {k}: max error {err:.3e}, bound {b[k]:.3e}, fraction {err / b[k]:.4f}")
        assert err <= b[k], (name, k, err, b[k])
    assert np.all(np.abs(r["l"] - m["l"]) <= U.bound(n, r["khi"], r["l"]))


@pytest.mark.parametrize("name", list(CASES))
def test_invariants(name):
    S, s, y, cens, r = _case(name)
    n = S.shape[0]
    W = (r["khi"] - r["klo"] + 1).astype(np.int64)
    for cls in (0, 1):
        sel = cens == cls
        # every p sums to 1 over its window: one unit of rounding per term,
        # and the rounding of p itself (4 operations on values <= 1)
        assert abs(int(r["words"][cls, :, 0].sum()) - int(sel.sum()) * 2 ** 40) <= int(W[sel].sum()) + 1
        assert np.all(r["words"][cls] >= 0)
    b = R.bounds(n, y, cens, r["klo"], r["khi"], np.ones(len(y), bool), r["yscale"])
    assert abs(r["Z"].sum() - y.sum()) <= n * b["Z"]
    assert abs(r["E"].sum() - (cens == 0).sum()) <= n * b["E"]
    assert abs(r["A"].sum() - (cens != 0).sum()) <= n * b["A"]
    assert np.all(r["Z"] >= 0) and np.all(r["N"] >= 0) and np.all(r["E"] >= 0) and np.all(r["A"] >= 0)
    assert np.all(np.diag(r["N"]) == 0) and np.all(r["N"][S == 0] == 0)
    # totals and pointwise l: the uniformisation evaluator's, bit for bit
    l = U.pointwise([S], [s], y, cens)[0]
    assert np.array_equal(l, r["l"])
    import loglik_ref as LR

    assert np.array_equal(LR.totals(l[None, :])[0], r["totals"])


def test_bad_observation_and_flagged_draw():
    S, s = bd_exit(3)
    y = np.array([0.5, 1.0, 1200.0, 2.0])  # mu y >= 2047 for the third
    cens = np.array([0, 1, 0, 0], np.int32)
    assert -S.diagonal().min() * 1200.0 >= 2047
    r = R.estep(S, s, y, cens)
    assert r["nbad"] == 1 and r["totals"][3] == 3 and r["loglik"] == -np.inf
    ok = R.estep(S, s, y[[0, 1, 3]], cens[[0, 1, 3]], yscale=r["yscale"], ymax=1200.0)
    assert np.array_equal(ok["words"], r["words"])  # counted, not added
    Sn = S.copy()
    Sn[1, 0] = np.nan
    f = R.estep(Sn, s, y, cens)
    assert f["flag"] == P.LL_F_NONFINITE and not f["words"].any() and np.isnan(f["loglik"])
    assert np.all(np.isnan(f["Z"])) and np.all(np.isnan(f["N"]))


def _loglik(S, s, y, cens):
    return float(np.sum(U.pointwise([S], [s], y, cens, ymax=float(np.max(y)))[0]))


@pytest.mark.parametrize("name", ["bd3", "bd10", "CYCLIC", "ring5", "ring10_s123_zero"])
def test_score_identity(name):
    """d l / d rate = N_ij / rate - Z_i (exit: E_i / s_i - Z_i) against the
    central difference D(h) = (l(r + h) - l(r - h)) / 2h, h = 1e-4 r.  The
    tolerance is the difference's own error, estimated from the step:
    truncation h^2 |l'''| / 6, taken from the same difference at 2h as
    |D(2h) - D(h)| / 3 (Richardson; doubled); rounding 2 B / 2h with B the
    a-priori bound of the restatement's l summed over the observations; plus
    the E-step's own bound on N / rate and Z."""
    S, s, y, cens, r = _case(name)
    n = S.shape[0]
    cells = [(i, j) for i in range(n) for j in range(n) if i != j and S[i, j] > 0][:3]
    cells.append((int(np.argmax(s)), n))
    b = R.bounds(n, y, cens, r["klo"], r["khi"], np.ones(len(y), bool), r["yscale"])
    B = float(np.sum(U.bound(n, r["khi"] + 8)))

    def moved(i, j, d):
        S2, s2 = S.copy(), s.copy()
        if j == n:
            s2[i] += d
        else:
            S2[i, j] += d
        S2[i, i] -= d
        return _loglik(S2, s2, y, cens)

    for (i, j) in cells:
        rate = s[i] if j == n else S[i, j]
        score = (r["E"][i] if j == n else r["N"][i, j]) / rate - r["Z"][i]
        h = 1e-4 * rate
        D1 = (moved(i, j, h) - moved(i, j, -h)) / (2 * h)
        D2 = (moved(i, j, 2 * h) - moved(i, j, -2 * h)) / (4 * h)
        tol = 2 * abs(D2 - D1) / 3 + B / h + (b["E"] if j == n else b["N"]) / rate + b["Z"]
        print(f"{name} ({i},{j}): score {score:.10g} fd {D1:.10g} diff {abs(score - D1):.2e} tol {tol:.2e}")
        assert abs(score - D1) <= tol, (name, i, j, score, D1, tol)


def test_shards_add_and_library_contract():
    S, s = bd_exit(10)
    y, cens = simulate_ph(S, s, 400, seed=5, censor_frac=0.3)
    ys = R.yscale_of(y.max())
    whole = R.hist(S, s, y, cens, yscale=ys)
    a = R.hist(S, s, y[:150], cens[:150], yscale=ys)
    b = R.hist(S, s, y[150:], cens[150:], yscale=ys)
    assert np.array_equal(a["words"] + b["words"], whole["words"])
    assert np.array_equal(a["totals"] + b["totals"], whole["totals"])
    for gen in ((S, s), U.ring(5), CASES["n1"]()):
        Sg, sg = gen
        yy, cc = simulate_ph(Sg, sg, 64, seed=6, censor_frac=0.3)
        h = R.hist(Sg, sg, yy, cc)
        ref = R.contract(Sg, sg, h["words"], h["yscale"])
        lib = P.estep_contract(Sg, sg, h["words"], h["yscale"])
        assert lib["flag"] == 0
        for k in "ZNEA":
            assert np.array_equal(lib[k], ref[k]), k
    with pytest.raises(P.PhaseTypeError):
        P.estep_contract(S, s, whole["words"], 3.0)  # not a power of two


def test_yscale():
    for v, want in ((1e-9, 2.0 ** -29), (1.0, 1.0), (1.0000001, 2.0), (100.0, 128.0), (0.5, 0.5), (0.0, 1.0)):
        assert R.yscale_of(v) == want
        assert P.load().pht_estep_yscale(v) == want


# ---- EM driven by the restatement
def _em_problem():
    """n = 3, 300 observations, 30 % censored; T ties S12 = S23 (parameter 1)
    and s1 = s2 (parameter 3), with C != 1 on one cell of each tie"""
    S, s = bd_exit(3)
    x, cens = simulate_ph(S, s, 300, seed=11, censor_frac=0.3)
    T = np.array([[0, 1, 0, 3], [2, 0, 1, 3], [0, 2, 0, 4], [0, 0, 0, 0]], np.int32)
    Cm = np.ones((4, 4))
    Cm[1, 2] = 2.5
    Cm[1, 3] = 0.4
    Cm[2, 1] = 1.7
    return x, cens, T, Cm


def _driver(x, cens):
    return lambda S, s: R.estep(S, s, x, cens)


@pytest.mark.parametrize("with_C", [False, True])
def test_em_monotone(with_C):
    x, cens, T, Cm = _em_problem()
    r = P.ph_em(x, T, cens, C_=Cm if with_C else None, start=[1.0, 0.7, 0.5, 1.5], iters=40, tol=0.0,
                estep=_driver(x, cens))
    ll = r["loglik"]
    assert r["iterations"] == 40 and len(ll) == 40 and not r["converged"]
    assert np.all(np.diff(ll) >= -len(x) * 2.0 ** -33), np.diff(ll).min()
    assert ll[-1] > ll[0] + 1.0
    S, s = P.theta_to_S(r["theta"], T, Cm if with_C else None)
    assert np.array_equal(S, r["S"]) and np.array_equal(s, r["s"])


def test_em_z_over_C_is_not_monotone():
    """the Gibbs update's quirk (z / C in place of C z) as an M-step does not
    maximise the likelihood when C != 1: the same run with it loses
    log-likelihood, which the monotonicity test above would catch"""
    x, cens, T, Cm = _em_problem()
    theta = np.array([1.0, 0.7, 0.5, 1.5])
    ll = []
    for _ in range(5):
        S, s = P.theta_to_S(theta, T, Cm)
        r = R.estep(S, s, x, cens)
        ll.append(r["loglik"])
        theta = P.em_step(T, 1.0 / Cm, r["Z"], r["N"], r["E"])
    assert np.all(np.isfinite(ll)) and np.diff(ll).min() < -1.0, ll


def test_em_map_rises_in_log_posterior():
    x, cens, T, Cm = _em_problem()
    nu, zeta = np.array([2.0, 1.5, 3.0, 2.0]), np.array([1.0, 2.0, 4.0, 1.0])
    r = P.ph_em(x, T, cens, C_=Cm, start=[1.0, 0.7, 0.5, 1.5], prior=(nu, zeta), iters=40, tol=0.0,
                estep=_driver(x, cens))
    assert np.all(np.diff(r["objective"]) >= -len(x) * 2.0 ** -33)
    ml = P.ph_em(x, T, cens, C_=Cm, start=[1.0, 0.7, 0.5, 1.5], iters=40, tol=0.0, estep=_driver(x, cens))
    assert not np.allclose(r["theta"], ml["theta"], rtol=1e-3)


def test_em_stops_and_fails_loudly():
    x, cens, T, Cm = _em_problem()
    r = P.ph_em(x, T, cens, start=[1.0, 0.7, 0.5, 1.5], iters=2000, tol=1e-7, estep=_driver(x, cens))
    assert r["converged"] and r["iterations"] < 2000
    with pytest.raises(P.PhaseTypeError):
        P.ph_em(x, T, cens, start=[1.0, np.inf, 0.5, 1.5], iters=3, estep=_driver(x, cens))
    with pytest.raises(P.PhaseTypeError):  # mu y beyond the table: a bad observation
        P.ph_em(x, T, cens, start=[1e4, 1e4, 1e4, 1e4], iters=3, estep=_driver(x, cens))
