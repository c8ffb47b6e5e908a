"""CPU: the fleet-condition specification (include/pht_condition.h) through the
tests' restatement (tests/condition_spec.c), the host-only library function and
the Python layer; no GPU.

* phi against the truth (mpmath) within the header's contract and nothing
  else; m and r_h within the header's recorded constants.
* Closed forms: the exponential, Erlang(n), c -> 0.
* Cross-checks against the evaluator, the forecast and the E-step.
* The flagged and bad paths, the exact reductions over shards, the refusals,
  pht_condition_host bit for bit, the exported symbols.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import condition_ref as Cd  # noqa: E402
import estep_ref as ES  # noqa: E402
import evaluator_cases as EC  # noqa: E402
import forecast_ref as F  # noqa: E402
import loglik_unif_ref as U  # noqa: E402
import phasetype_amd as P  # noqa: E402
from phasetype_amd.synth import bd_exit  # noqa: E402

CASES = {
    "bd3": lambda: bd_exit(3),
    "bd10": lambda: bd_exit(10),
    "erlang3": lambda: EC.erlang(3),
    "ring5": lambda: U.ring(5),
    "stiff6": lambda: EC.stiff(6),
}
CASES.update(EC.TRUTH_CASES)  # the chain families, the structures and a stiffer table (evaluator_cases)
AGES = np.array([1e-6, 1e-3, 0.1, 1.0, 5.0, 20.0])
HORIZONS = np.array([0.0, 1e-9, 0.1, 1.0, 10.0])
ULP = 2.0 ** -53


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _mu(S):
    return float(np.max(-np.diag(S)))


def _ages(S):
    """AGES within the evaluator's range for this generator"""
    return AGES[_mu(S) * AGES <= EC.MU_Y_MAX]


def _ones(k):
    return np.ones(k, np.int32)


def _f(rows):
    return np.array([[float(v) for v in row] for row in rows])


# ----------------------------------------------- contract, recorded constants
@pytest.mark.parametrize("name", list(CASES))
def test_phi_within_the_headers_contract(name):
    import mpmath as mp

    S, s = CASES[name]()
    ages = _ages(S)
    r = Cd.condition([S], [s], ages, _ones(len(ages)))
    assert r["flags"][0] == 0 and r["nbad"][0] == 0 and r["nunits"][0] == len(ages)
    _, bad, khi = Cd.windows(S, s, ages)
    truth = Cd.truth_phi(S, ages)
    worst = 0.0
    for i in range(len(ages)):
        for j in range(S.shape[0]):
            b = Cd.spec().cspec_phi_bound(S.shape[0], int(khi[i]), float(truth[i][j]))
            e = float(abs(mp.mpf(float(r["phi"][0, i, j])) - truth[i][j]))
            worst = max(worst, e / b)
            assert e <= b, (name, ages[i], j, e, b)
    print(f"{name}: largest error / bound {worst:.4f}")


@pytest.mark.parametrize("name", list(CASES))
def test_m_and_r_within_the_recorded_constants(name):
    import mpmath as mp

    S, s = CASES[name]()
    mu = _mu(S)
    m, flag = Cd.mean(S, s)
    assert flag == 0
    em = max(float(abs((mp.mpf(float(a)) - b) / b)) for a, b in zip(m, Cd.truth_m(S)))
    h = np.geomspace(1e-6, 1e3, 10) / mu
    r, Kr, flag = Cd.renewal(S, s, h)
    assert flag == 0 and Kr < 2047
    rt = Cd.truth_r(S, s, h)
    worst = 0.0
    for j, hj in enumerate(h):
        b = Cd.spec().cspec_r_bound(mu * hj)
        e = max(float(abs((mp.mpf(float(a)) - t) / t)) for a, t in zip(r[j], rt[j]))
        worst = max(worst, e / b)
        assert e <= b, (name, hj, e, b)
    print(f"{name}: m error {em / ULP:.2f} x 2^-53 (recorded {Cd.spec().cspec_m_r() / ULP:.0f}), "
          f"r error / recorded bound {worst:.3f}")
    assert em <= Cd.spec().cspec_m_r()


def test_truth_is_resolved_or_refused():
    """Erlang(10) at mu h = 1e-6: r_h[0] = x^10 / 10! (1 + O(x)) = 3e-67.  At a
    fixed 60 digits the helper must refuse; at its own precision it gives the
    closed form's leading term.  m of the same chain is (n - i) / lam"""
    import mpmath as mp

    n, x = 10, 1e-6
    S, s = EC.erlang(n)
    h = [x / _mu(S)]
    with pytest.raises(AssertionError, match="does not resolve"):
        Cd.truth_r(S, s, h, dps=60)
    assert Cd.truth_r_dps(n, x) == 60 + 3 * n * 6
    r = Cd.truth_r(S, s, h)
    with mp.workdps(60):
        xm = mp.mpf(_mu(S)) * mp.mpf(h[0])
        assert abs(r[0][0] / (xm ** n / mp.factorial(n)) - 1) < 2 * x
        assert abs(r[0][n - 1] / xm - 1) < 2 * x
        m = Cd.truth_m(S)
        assert all(abs(m[i] * mp.mpf(EC.LAM) / (n - i) - 1) < mp.mpf(10) ** -50 for i in range(n))


def test_issue_orientation_values():
    S, s = bd_exit(3)
    r = Cd.condition([S], [s], [2.0], [1], [0.1, 1.0, 10.0])
    assert abs(r["mrl"][0, 0] - 0.88524) < 5e-6
    assert np.allclose(r["d"][0, 0], [0.1051, 0.8636, 7.646], rtol=5e-4)
    q = F.forecast([S], [s], [2.0], [1], [0.1, 1.0, 10.0])["q"][0, 0]
    assert np.allclose(q, [0.1035, 0.6745, 0.99999], rtol=5e-4)


# --------------------------------------------------------------- closed forms
def test_exponential():
    lam = 1.7
    S, s = np.array([[-lam]]), np.array([lam])
    ages, h = np.array([0.0, 0.3, 2.0, 9.0]), np.array([0.0, 0.5, 3.0])
    r = Cd.condition([S], [s], ages, _ones(4), h)
    assert r["nbad"][0] == 0 and np.all(r["phi"] == 1.0)
    assert np.all(np.abs(r["mrl"][0] - 1.0 / lam) <= 2 * ULP / lam)
    # D(h) = lam h, whatever the age: within the recorded bound of r_h and the dot's rounding
    for j, hj in enumerate(h):
        tol = (Cd.spec().cspec_r_bound(lam * hj) + 4 * ULP) * lam * hj
        assert np.all(np.abs(r["d"][0, :, j] - lam * hj) <= tol), (hj, r["d"][0, :, j])


@pytest.mark.parametrize("n", [3, 6])
def test_erlang(n):
    import mpmath as mp

    lam = EC.LAM
    S, s = EC.erlang(n, lam)
    m, flag = Cd.mean(S, s)
    assert flag == 0
    want = (n - np.arange(n)) / lam
    assert np.all(np.abs(m - want) <= Cd.spec().cspec_m_r() * want)
    ages = np.array([1e-3, 0.7, 4.0, 15.0])
    r = Cd.condition([S], [s], ages, _ones(4))
    _, _, khi = Cd.windows(S, s, ages)
    for i, c in enumerate(ages):
        w = [(mp.mpf(lam) * mp.mpf(float(c))) ** j / mp.factorial(j) for j in range(n)]
        tot = mp.fsum(w)
        for j in range(n):
            t = w[j] / tot
            assert float(abs(mp.mpf(float(r["phi"][0, i, j])) - t)) <= Cd.spec().cspec_phi_bound(n, int(khi[i]), float(t))


@pytest.mark.parametrize("name", ["bd3", "ring5"])
def test_age_zero_is_the_first_phase(name):
    S, s = CASES[name]()
    r = Cd.condition([S], [s], np.array([0.0, 1.0]), _ones(2))
    e1 = np.zeros(S.shape[0])
    e1[0] = 1.0
    assert np.array_equal(r["phi"][0, 0], e1) and r["nbad"][0] == 0
    m, _ = Cd.mean(S, s)
    assert r["mrl"][0, 0] == m[0]


# --------------------------------------------------------------- cross-checks
@pytest.mark.parametrize("name", list(CASES))
def test_phi_sums_to_one(name):
    S, s = CASES[name]()
    ages = np.concatenate([_ages(S), np.linspace(0.05, 3.0, 40)])
    r = Cd.condition([S], [s], ages, _ones(len(ages)))
    assert np.all(np.abs(r["phi"][0].sum(1) - 1.0) <= S.shape[0] * 2.0 ** -52)
    assert np.all(r["phi"] >= 0.0)


@pytest.mark.parametrize("name", list(CASES))
def test_window_is_the_evaluators_and_the_forecasts(name):
    """l of pht_es_window at the age = pht_llu_eval's, which is pht_fc_draw's l0
    (the forecast at h = 0 sizes its table for the same y_max); the bad set is
    the forecast's at h = 0, with ages beyond the table among them"""
    S, s = CASES[name]()
    ages = np.concatenate([_ages(S), [1800.0 / _mu(S), 5000.0 / _mu(S)]])
    l, bad, _ = Cd.windows(S, s, ages)
    lu = U.pointwise([S], [s], ages, _ones(len(ages)))[0]
    assert _bits(l) == _bits(lu)
    r = Cd.condition([S], [s], ages, _ones(len(ages)))
    f = F.forecast([S], [s], ages, _ones(len(ages)), [0.0])
    assert np.array_equal(np.isnan(r["mrl"][0]), np.isnan(f["q"][0, :, 0]))
    assert np.array_equal(np.isnan(r["mrl"][0]), bad != 0) and bad.sum() >= 1
    assert r["nbad"][0] == f["nbad"][0, 0] == bad.sum()
    assert np.array_equal(r["cnt"], 1 - bad) and np.all(np.isnan(r["phi"][0][bad != 0]))


@pytest.mark.parametrize("name", ["bd3", "bd10", "ring5"])
def test_sum_over_units_is_the_esteps_A(name):
    S, s = CASES[name]()
    n = S.shape[0]
    rng = np.random.default_rng(3)
    y = np.round(rng.exponential(2.0, 60), 3) + 0.001
    cens = (rng.random(60) < 0.5).astype(np.int32)
    e = ES.estep(S, s, y, cens)
    good = ~np.isnan(e["l"])
    assert good.all()
    b_es = ES.bounds(n, y, cens, e["klo"], e["khi"], good, e["yscale"])["A"]
    # the condition's table is sized for the largest censored age, the E-step's for the largest observation
    r = Cd.condition([S], [s], y, cens, ymax_c=float(np.max(y)))
    _, _, khi = Cd.windows(S, s, y[cens != 0], ymax_c=float(np.max(y)))
    b_cd = sum(Cd.spec().cspec_phi_bound(n, int(k), 1.0) for k in khi)
    got = r["phi"][0].sum(0)
    assert np.all(np.abs(got - e["A"]) <= b_es + b_cd + n * len(khi) * ULP), (got - e["A"], b_es, b_cd)
    # and the fixed-point words are that sum, each unit rounded once to 2^-40
    assert np.all(np.abs(r["Phi"][0] - got) <= len(khi) * 2.0 ** -41 + len(khi) * ULP)


@pytest.mark.parametrize("name", list(CASES))
def test_demand_against_the_first_failure_probability(name):
    """with replacement no fewer failures are expected than the probability of
    a first one; the two agree to O((mu h)^2) at a short horizon; D increases"""
    S, s = CASES[name]()
    n, mu = S.shape[0], _mu(S)
    ages = _ages(S)
    h = np.concatenate([[1e-6 / mu], np.geomspace(1e-3, 50.0, 9) / mu])
    r = Cd.condition([S], [s], ages, _ones(len(ages)), h)
    f = F.forecast([S], [s], ages, _ones(len(ages)), h)
    assert r["nbad"][0] == 0 and not f["nbad"].any()
    D, q = r["d"][0], f["q"][0]
    _, _, khi = Cd.windows(S, s, ages)
    rr, _, _ = Cd.renewal(S, s, h)
    # |D^ - D| <= sum_j |dphi_j| r_j + (r's recorded bound + the dot's n + 2 roundings) D
    tol_d = np.array([[sum(Cd.spec().cspec_phi_bound(n, int(khi[i]), float(min(1.0, 1.01 * r["phi"][0, i, k])))
                           * rr[j, k] for k in range(n))
                       + (Cd.spec().cspec_r_bound(mu * h[j]) + (n + 2) * ULP) * D[i, j]
                       for j in range(len(h))] for i in range(len(ages))])
    tol_q = F.bound(S, s, ages, h, q)
    assert np.all(D >= q - tol_d - tol_q)
    assert np.all(D[:, 0] - q[:, 0] <= (mu * h[0]) ** 2 + tol_d[:, 0] + tol_q[:, 0])
    assert np.all(np.diff(D, axis=1) > 0)


# -------------------------------------------------------- flagged, bad paths
def test_flagged_draws_are_skipped():
    S, s = bd_exit(3)
    trap = S.copy()  # state 3 neither moves nor exits
    st = s.copy()
    trap[2, :] = 0.0
    st[2] = 0.0
    loop = S.copy()  # states 2 and 3 only reach each other
    sl = s.copy()
    loop[1, :] = [0.0, -2.0, 2.0]
    loop[2, :] = [0.0, 3.0, -3.0]
    sl[1] = sl[2] = 0.0
    Sn = S.copy()
    Sn[2, 1] = np.nan
    ages, h = np.array([0.5, 2.0]), np.array([0.5, 2.0])
    r = Cd.condition([S, trap, loop, Sn, 1.1 * S], [s, st, sl, s, 1.1 * s], ages, _ones(2), h)
    assert r["flags"].tolist() == [0, 64, 64, 4, 0] and Cd.spec().cspec_f_trap() == P.CD_F_TRAP == 64
    for d in (1, 2, 3):
        assert not r["words"][d].any() and not r["scales"][d].any()
        assert np.all(np.isnan(r["phi"][d])) and np.all(np.isnan(r["mrl"][d])) and np.all(np.isnan(r["d"][d]))
    assert r["cnt"].tolist() == [2, 2] and r["nunits"].tolist() == [2, 0, 0, 0, 2]
    # the sums are those of the two good draws alone
    g = Cd.condition([S, 1.1 * S], [s, 1.1 * s], ages, _ones(2), h)
    for k in ("phisum", "mrlsum", "dsum"):
        assert _bits(r[k]) == _bits(g[k]), k


def test_horizon_beyond_the_renewal_table():
    S, s = bd_exit(3)
    mu = _mu(S)
    ages = np.array([0.5, 2.0])
    ok = Cd.condition([S], [s], ages, _ones(2), [1.0, 1400.0 / mu])
    assert ok["flags"][0] == 0 and np.all(np.isfinite(ok["d"]))
    r = Cd.condition([S, 0.5 * S], [s, 0.5 * s], ages, _ones(2), [1.0, 1600.0 / mu])
    assert r["flags"].tolist() == [128, 0] and Cd.spec().cspec_f_hcap() == P.CD_F_HCAP == 128
    assert not r["words"][0].any() and np.all(np.isnan(r["phi"][0])) and r["cnt"].tolist() == [1, 1]
    # without horizons the same draw is usable
    assert Cd.condition([S], [s], ages, _ones(2))["flags"][0] == 0


def test_age_beyond_the_table_is_bad():
    S, s = bd_exit(3)
    ages = np.array([1.0, 3000.0 / _mu(S), 2.0])
    r = Cd.condition([S, 0.9 * S], [s, 0.9 * s], ages, _ones(3), [1.0])
    assert r["nbad"].tolist() == [1, 1] and r["nunits"].tolist() == [2, 2] and r["cnt"].tolist() == [2, 0, 2]
    assert np.all(np.isnan(r["phi"][:, 1])) and np.all(np.isnan(r["mrl"][:, 1])) and np.all(np.isnan(r["d"][:, 1]))
    assert not r["phisum"][1].any() and r["mrlsum"][1] == 0 and not r["dsum"][1].any()
    assert np.isnan(r["p_phase"][1]).all() and np.isfinite(r["p_phase"][[0, 2]]).all()


# ----------------------------------------------------- reductions, plumbing
def test_words_add_over_shards():
    S, s = bd_exit(5)
    Ss, ss = [S * c for c in (0.8, 1.0, 1.25)], [s * c for c in (0.8, 1.0, 1.25)]
    rng = np.random.default_rng(8)
    y = np.round(rng.exponential(3.0, 100), 2) + 0.01
    cens = (rng.random(100) < 0.6).astype(np.int32)
    whole = Cd.condition(Ss, ss, y, cens, HORIZONS)
    a = Cd.condition(Ss, ss, y[:50], cens[:50], HORIZONS)  # each shard's table from its own largest censored age
    b = Cd.condition(Ss, ss, y[50:], cens[50:], HORIZONS)
    assert np.array_equal(a["words"] + b["words"], whole["words"]) and np.array_equal(a["scales"], whole["scales"])
    c = P.condition_combine(a, b)
    for k in ("words", "scales", "Phi", "L", "Delta", "nbad", "nunits", "phisum", "mrlsum", "dsum", "cnt", "p_phase",
              "mrl_unit", "demand_unit", "phi", "mrl", "d"):
        assert _bits(c[k]) == _bits(whole[k]), k
    assert np.allclose(whole["Phi"].sum(1), whole["nunits"], rtol=0, atol=1e-9)
    with pytest.raises(ValueError, match="same draws"):
        P.condition_combine(a, Cd.condition(Ss[:2], ss[:2], y[50:], cens[50:], HORIZONS))


@pytest.mark.parametrize("name,nh", [("bd3", 0), ("bd10", 5), ("ring5", 1), ("stiff6", 5)])
def test_host_function_is_the_restatement(lib, name, nh):
    S, s = CASES[name]()
    ages = _ages(S)
    h = HORIZONS[:nh]
    Ss, ss = [S, 1.1 * S], [s, 1.1 * s]
    want = Cd.condition(Ss, ss, ages, _ones(len(ages)), h)
    st = None
    for d in range(2):
        st = P.condition_host(Ss[d], ss[d], ages, h, state=st)
        for k in ("words", "scales", "phi", "mrl", "d", "Phi", "L", "Delta"):
            assert _bits(st[k][0]) == _bits(want[k][d]), (k, d)
    for k in ("phisum", "mrlsum", "dsum", "cnt", "p_phase", "mrl_unit", "demand_unit"):
        assert _bits(st[k]) == _bits(want[k]), k


def test_host_function_refusals(lib):
    S, s = bd_exit(3)
    ok = np.array([1.0, 2.0])
    P.condition_host(S, s, ok, [0.5])
    with pytest.raises(P.PhaseTypeError, match="no censored unit"):
        P.condition_host(S, s, np.zeros(0))
    for h in (np.arange(17.0), [-1.0], [np.nan], [1.0, np.inf], [1.0, 1.0], [2.0, 1.0]):
        with pytest.raises(P.PhaseTypeError, match="horizon"):
            P.condition_host(S, s, ok, h)
    with pytest.raises(P.PhaseTypeError, match="at most"):
        P.condition_host(S, s, np.ones((1 << 22) + 1))
    with pytest.raises(P.PhaseTypeError, match="ymax_c"):
        P.condition_host(S, s, ok, [0.5], ymax_c=1.5)
    r = P.condition_host(S, s, ok, np.arange(16.0))
    assert r["d"].shape == (1, 2, 16) and r["words"].shape == (1, 3 + 16 + 3)
    assert P.condition_host(S, s, ok)["d"].shape == (1, 2, 0)


def test_exports(lib):
    names = ["pht_ctx_condition", "pht_ctx_condition_grid_cap", "pht_ctx_condition_ms", "pht_condition_host"]
    src = open(os.path.join(os.path.dirname(HERE), "include", "phasetype_amd.h")).read()
    for name in names:
        assert name in P.EXPORTS and hasattr(lib, name) and (name + "(") in src, name
    assert Cd.spec().cspec_maxunits() == P.CONDITION_MAX_UNITS and Cd.spec().cspec_maxh() == P.CONDITION_MAX_H
    assert Cd.spec().cspec_scale() == 2.0 ** 40
