"""CPU: the fleet-spares specification (include/pht_spares.h) through the tests'
restatement (tests/spares_spec.c), the host-only library function and the
Python layer; no GPU.

* r_h bit for bit pht_cd_renewal's; q_h and var against the truth (mpmath)
  within the header's recorded constants.
* Closed forms: the exponential, Erlang-2.  A fixed-seed simulation of the
  replacement process.
* h = 0, no negative variance, the exact reductions over shards, state=,
  pht_spares_host bit for bit, the refusals, the exported symbols.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import condition_ref as Cd  # noqa: E402
import evaluator_cases as EC  # noqa: E402
import loglik_unif_ref as U  # noqa: E402
import phasetype_amd as P  # noqa: E402
import spares_ref as Sp  # noqa: E402
from phasetype_amd.synth import bd_exit  # noqa: E402

CASES = {
    "bd3": lambda: bd_exit(3),
    "bd10": lambda: bd_exit(10),
    "erlang3": lambda: EC.erlang(3),
    "ring5": lambda: U.ring(5),
    "stiff6": lambda: EC.stiff(6),
}
CASES.update(EC.TRUTH_CASES)  # the chain families, the structures and a stiffer table (evaluator_cases)
HORIZONS = np.array([0.0, 1e-9, 0.1, 1.0, 10.0])
ULP = 2.0 ** -53


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _mu(S):
    return float(np.max(-np.diag(S)))


def _ones(k):
    return np.ones(k, np.int32)


def _hs(S):
    """HORIZONS, shrunk where mu is large so that mu h stays at 100 at most"""
    return HORIZONS * min(1.0, 10.0 / _mu(S))


def _grid(S):
    """the header's grid of horizons: 1e-6 .. 1e3 / mu"""
    return np.geomspace(1e-6, 1e3, 10) / _mu(S)


# --------------------------------------------------- the draw's moment vectors
@pytest.mark.parametrize("name", list(CASES))
def test_renewal_columns_are_the_conditions(name):
    S, s = CASES[name]()
    for h in (_grid(S), _hs(S), np.array([0.7 / _mu(S)])):
        r, _, scales, Kr, flag = Sp.vectors(S, s, h)
        rc, Krc, flagc = Cd.renewal(S, s, h)
        assert flag == 0 and flagc == 0 and Kr == Krc
        assert _bits(r) == _bits(rc)
        # and the first half of the scales is the condition's dscale
        c = Cd.condition([S], [s], [1.0], [1], h)
        assert _bits(scales[:len(h)]) == _bits(c["scales"][0, 1:])


@pytest.mark.parametrize("name", list(CASES))
def test_q_and_var_within_the_recorded_constants(name):
    """on the columns (phi = e_i exact): q_h relative to itself, var relative to
    Q + D + D^2 (what the cancellation in Q + D - D^2 leaves)"""
    import mpmath as mp

    S, s = CASES[name]()
    mu, h = _mu(S), _grid(S)
    r, q, _, Kr, flag = Sp.vectors(S, s, h)
    assert flag == 0 and Kr < 2047
    v = Sp.var(r, q)
    m1, m2 = Sp.truth_moments(S, s, h)
    wq = wv = lost = 0.0
    for j, hj in enumerate(h):
        bq = Sp.spec().sspec_q_bound(mu * hj)
        for i in range(S.shape[0]):
            D, Q = m1[j][i], m2[j][i]
            eq = float(abs((mp.mpf(float(q[j, i])) - Q) / Q))
            vt = Q + D - D * D
            ev = float(abs(mp.mpf(float(v[j, i])) - vt))
            bv = Sp.spec().sspec_var_bound(mu * hj, float(D), float(Q))
            wq, wv, lost = max(wq, eq / bq), max(wv, ev / bv), max(lost, ev / float(vt))
            assert eq <= bq, (name, hj, i, eq, bq)
            assert ev <= bv, (name, hj, i, ev, bv)
    print(f"{name}: q error / recorded bound {wq:.3f}, var error / recorded bound {wv:.3f}, "
          f"largest relative error of var {lost / ULP:.3g} x 2^-53")


def test_truth_is_resolved_or_refused():
    """Erlang(10) at mu h = 1e-5: q_h[0] = 2 x^20 / 20! (1 + O(x)) = 8e-119.  At
    a fixed 60 digits the helper must refuse; at its own precision it gives
    the closed form's leading term"""
    import mpmath as mp

    n, x = 10, 1e-5
    S, s = EC.erlang(n)
    h = [x / _mu(S)]
    with pytest.raises(AssertionError, match="does not resolve"):
        Sp.truth_moments(S, s, h, dps=60)
    assert Sp.truth_dps(n, x) == 60 + 6 * n * 5
    m1, m2 = Sp.truth_moments(S, s, h)
    with mp.workdps(60):
        xm = mp.mpf(_mu(S)) * mp.mpf(h[0])
        assert abs(m2[0][0] / (2 * xm ** (2 * n) / mp.factorial(2 * n)) - 1) < 2 * x
        assert abs(m1[0][0] / (xm ** n / mp.factorial(n)) - 1) < 2 * x
        assert abs(m1[0][n - 1] / xm - 1) < 2 * x


@pytest.mark.parametrize("name", ["bd3", "ring5"])
def test_a_units_var_within_the_constants_and_phis_contract(name):
    """a unit of age c: what phi's own error (the condition's contract) moves,
    sum_j |dphi_j| (q_j + r_j + 2 D r_j), and the n + 2 roundings of each dot,
    (n + 2) 2^-53 (Q + D + 2 D^2), on top of the recorded bound"""
    import mpmath as mp

    S, s = CASES[name]()
    n, mu = S.shape[0], _mu(S)
    ages, h = np.array([1e-3, 1.0, 20.0]), np.array([1e-3, 1.0, 30.0]) / mu
    got = Sp.spares([S], [s], ages, _ones(3), h)
    assert got["flags"][0] == 0 and got["nbad"][0] == 0
    _, _, khi = Cd.windows(S, s, ages)
    phi = Cd.truth_phi(S, ages)
    m1, m2 = Sp.truth_moments(S, s, h)
    for i in range(3):
        for j, hj in enumerate(h):
            D = mp.fsum(p * a for p, a in zip(phi[i], m1[j]))
            Q = mp.fsum(p * a for p, a in zip(phi[i], m2[j]))
            vt = Q + D - D * D
            Df, Qf = float(D), float(Q)
            tol = Sp.spec().sspec_var_bound(mu * hj, Df, Qf) + (n + 2) * ULP * (Qf + Df + 2 * Df * Df) + \
                sum(Cd.spec().cspec_phi_bound(n, int(khi[i]), float(phi[i][k]))
                    * float(m2[j][k] + m1[j][k] + 2 * D * m1[j][k]) for k in range(n))
            e = float(abs(mp.mpf(float(got["var"][0, i, j])) - vt))
            assert e <= tol, (name, ages[i], hj, e, tol)
            assert abs(got["d"][0, i, j] - Df) <= (Cd.spec().cspec_r_bound(mu * hj) + (n + 2) * ULP) * Df + \
                sum(Cd.spec().cspec_phi_bound(n, int(khi[i]), float(phi[i][k])) * float(m1[j][k]) for k in range(n))


# --------------------------------------------------------------- closed forms
def test_exponential():
    """n = 1, rate lam: a Poisson process whatever the age; mean = var = lam h
    and E N (N - 1) = (lam h)^2"""
    lam = 1.7
    S, s = np.array([[-lam]]), np.array([lam])
    ages, h = np.array([0.0, 0.3, 2.0, 9.0]), np.array([0.0, 0.5, 3.0, 40.0])
    r, q, _, _, flag = Sp.vectors(S, s, h)
    assert flag == 0
    got = Sp.spares([S], [s], ages, _ones(4), h)
    assert got["nbad"][0] == 0
    for j, hj in enumerate(h):
        x = lam * hj
        assert abs(r[j, 0] - x) <= Cd.spec().cspec_r_bound(x) * x
        assert abs(q[j, 0] - x * x) <= Sp.spec().sspec_q_bound(x) * x * x
        # phi = 1 exactly, one rounding in each dot
        assert np.all(np.abs(got["d"][0, :, j] - x) <= (Cd.spec().cspec_r_bound(x) + 4 * ULP) * x)
        tol = Sp.spec().sspec_var_bound(x, x, x * x) + 4 * ULP * (x + 3 * x * x)
        assert np.all(np.abs(got["var"][0, :, j] - x) <= tol), (hj, got["var"][0, :, j] - x, tol)


@pytest.mark.parametrize("x", [0.13, 1.3, 13.0, 3.9])
def test_erlang2(x):
    """Erlang-2 of rate lam, a new unit, x = lam h:
    mean = x / 2 - 1 / 4 + exp(-2 x) / 4,
    var = x / 4 + 1 / 16 - (x / 2) exp(-2 x) - exp(-4 x) / 16"""
    import mpmath as mp

    lam = 0.8
    S, s = EC.erlang(2, lam)
    mu, h = _mu(S), x / lam
    got = Sp.spares([S], [s], [0.0], [1], [h])
    with mp.workdps(40):
        xm = mp.mpf(lam) * mp.mpf(h)
        mean = xm / 2 - mp.mpf(1) / 4 + mp.exp(-2 * xm) / 4
        var = xm / 4 + mp.mpf(1) / 16 - (xm / 2) * mp.exp(-2 * xm) - mp.exp(-4 * xm) / 16
        Q = var - mean + mean * mean
        em = float(abs(mp.mpf(float(got["d"][0, 0, 0])) - mean))
        ev = float(abs(mp.mpf(float(got["var"][0, 0, 0])) - var))
    # age 0: phi = e_1 exactly
    assert em <= (Cd.spec().cspec_r_bound(mu * h) + 4 * ULP) * float(mean)
    assert ev <= Sp.spec().sspec_var_bound(mu * h, float(mean), float(Q)) + 4 * ULP * float(Q + mean + 2 * mean * mean)


def _simulate(S, s, phi, h, paths, rng):
    """the number of failures within h of a unit replaced at failure that
    starts in a phase drawn from phi, per path"""
    n = S.shape[0]
    rate = -np.diag(S)
    jump = np.concatenate([np.where(np.eye(n, dtype=bool), 0.0, S), s[:, None]], axis=1) / rate[:, None]
    cum = np.cumsum(jump, axis=1)
    state = rng.choice(n, size=paths, p=phi / phi.sum())
    t, count = np.zeros(paths), np.zeros(paths, np.int64)
    live = np.arange(paths)
    while len(live):
        st = state[live]
        t[live] += rng.exponential(1.0, len(live)) / rate[st]
        live = live[t[live] <= h]
        st = state[live]
        nxt = (rng.random(len(live))[:, None] >= cum[st]).sum(1)
        fail = nxt >= n
        count[live[fail]] += 1
        state[live] = np.where(fail, 0, np.minimum(nxt, n - 1))
    return count


def test_monte_carlo_of_the_replacement_process():
    """3 units at distinct ages on bd_exit(3), 2 10^5 paths each from the
    specification's phi: the fleet's count is the sum of the three.  Mean
    within 5 standard errors; variance within 5 standard errors of the sample
    variance, that error from the sample's fourth moment."""
    S, s = bd_exit(3)
    ages, h, N = np.array([0.2, 1.5, 4.0]), 4.0, 200_000
    got = Sp.spares([S], [s], ages, _ones(3), [h])
    phi = Cd.condition([S], [s], ages, _ones(3))["phi"][0]
    rng = np.random.default_rng(20240611)
    total = sum(_simulate(S, s, phi[i], h, N, rng) for i in range(3)).astype(np.float64)
    mean, dev = total.mean(), total - total.mean()
    var, m4 = np.mean(dev ** 2), np.mean(dev ** 4)
    se_mean, se_var = np.sqrt(var / N), np.sqrt((m4 - var * var) / N)
    print(f"mean {got['Delta'][0, 0]:.5f} vs {mean:.5f} (se {se_mean:.5f}), "
          f"variance {got['V'][0, 0]:.5f} vs {var:.5f} (se {se_var:.5f})")
    assert abs(got["Delta"][0, 0] - mean) <= 5 * se_mean
    assert abs(got["V"][0, 0] - var) <= 5 * se_var
    # the words are the three units', each rounded once to 2^-40 of its scale
    assert abs(got["V"][0, 0] - got["var"][0, :, 0].sum()) <= 3 * 2.0 ** -41 * got["scales"][0, 1] + 4 * ULP * var


# ----------------------------------------------------------- edges of the range
@pytest.mark.parametrize("name", list(CASES))
def test_zero_horizon_is_exactly_zero(name):
    S, s = CASES[name]()
    got = Sp.spares([S], [s], [0.0, 0.5, 2.0], _ones(3), [0.0, 1.0])
    assert got["nbad"][0] == 0
    assert _bits(got["d"][0, :, 0]) == _bits(np.zeros(3)) and _bits(got["var"][0, :, 0]) == _bits(np.zeros(3))
    assert got["words"][0, 0] == 0 and got["words"][0, 2] == 0 and got["Delta"][0, 0] == 0 and got["V"][0, 0] == 0
    assert np.all(got["d"][0, :, 1] > 0) and np.all(got["var"][0, :, 1] > 0)
    r, q, _, _, _ = Sp.vectors(S, s, [0.0, 1.0])
    assert not r[0].any() and not q[0].any()


def test_no_negative_variance():
    """the truth is positive at any h > 0; at the shortest horizon var = D up
    to the second order in h; at the longest (mu h = 1400 on Erlang(3), D = 467, D^2 = 2 10^5)
    what the cancellation leaves is the renewal asymptote lam h / 9 + O(1)"""
    for name in CASES:
        S, s = CASES[name]()
        r, q, _, _, flag = Sp.vectors(S, s, [1e-9 / _mu(S)])
        v = Sp.var(r, q)
        # every failure restarts in phase 1 or later: Q <= 2 D max r and D^2 <= D max r
        assert flag == 0 and np.all(v > 0) and np.all(np.abs(v - r) <= (3 * np.max(r) + 4 * ULP) * r)
    S, s = EC.erlang(3)
    mu = _mu(S)
    r, q, _, Kr, flag = Sp.vectors(S, s, [1400.0 / mu])
    assert flag == 0 and Kr < 2047
    v = Sp.var(r, q)
    # a renewal process of Erlang(3) lifetimes: Var N(t) -> t sigma^2 / m^3 + const = lam t / 9 + O(1)
    assert np.all(v > 0) and np.all(np.abs(v - 1400.0 / 9.0) < 1.0), v
    ages = np.array([0.0, 1.0, 50.0])
    got = Sp.spares([S], [s], ages, _ones(3), [1e-9 / mu, 1400.0 / mu])
    assert got["nbad"][0] == 0 and np.all(got["var"] > 0) and np.all(got["V"] > 0)


def test_flagged_draws_are_the_conditions():
    S, s = bd_exit(3)
    trap, st = S.copy(), s.copy()  # state 3 neither moves nor exits
    trap[2, :] = 0.0
    st[2] = 0.0
    Sn = S.copy()
    Sn[2, 1] = np.nan
    mu = _mu(S)
    ages, h = np.array([0.5, 2.0]), np.array([0.5, 1500.0 / mu])
    Ss, ss = [S, trap, Sn, 0.5 * S, 1.1 * S], [s, st, s, 0.5 * s, 1.1 * s]
    got = Sp.spares(Ss, ss, ages, _ones(2), h)
    cond = Cd.condition(Ss, ss, ages, _ones(2), h)
    assert got["flags"].tolist() == [128, 64 | 128, 4, 0, 128] and np.array_equal(got["flags"], cond["flags"])
    for d in (0, 1, 2, 4):
        assert not got["words"][d].any() and not got["scales"][d].any()
        assert np.all(np.isnan(got["d"][d])) and np.all(np.isnan(got["var"][d]))
    assert got["cnt"].tolist() == [1, 1] and got["nunits"].tolist() == [0, 0, 0, 2, 0]
    assert _bits(got["d"]) == _bits(cond["d"]) and _bits(got["dsum"]) == _bits(cond["dsum"])
    assert _bits(got["Delta"]) == _bits(cond["Delta"])
    # a unit beyond the table is bad: counted, never summed
    far = Sp.spares([S], [s], np.array([1.0, 3000.0 / mu]), _ones(2), [1.0])
    assert far["nbad"].tolist() == [1] and far["cnt"].tolist() == [1, 0] and np.all(np.isnan(far["var"][0, 1]))
    assert not far["vsum"][1].any() and np.isnan(far["demand_unit_sd"][1, 0])


# ----------------------------------------------------- reductions, plumbing
def test_words_add_over_shards():
    S, s = bd_exit(5)
    Ss, ss = [S * c for c in (0.8, 1.0, 1.25)], [s * c for c in (0.8, 1.0, 1.25)]
    rng = np.random.default_rng(8)
    y = np.round(rng.exponential(3.0, 100), 2) + 0.01
    cens = (rng.random(100) < 0.6).astype(np.int32)
    whole = Sp.spares(Ss, ss, y, cens, HORIZONS)
    a = Sp.spares(Ss, ss, y[:50], cens[:50], HORIZONS)
    b = Sp.spares(Ss, ss, y[50:], cens[50:], HORIZONS)
    assert np.array_equal(a["words"] + b["words"], whole["words"]) and np.array_equal(a["scales"], whole["scales"])
    c = P.spares_combine(a, b)
    for k in Sp.ALL:
        if k != "unit_index":
            assert _bits(c[k]) == _bits(whole[k]), k
    # the per-unit sd is the law of total variance over the draws
    k = whole["cnt"][:, None]
    want = np.sqrt(whole["var"].mean(0) + whole["d"].var(0))
    assert np.all(k == 3) and np.allclose(whole["demand_unit_sd"], want, rtol=1e-9, atol=1e-12)
    with pytest.raises(ValueError, match="same draws"):
        P.spares_combine(a, Sp.spares(Ss[:2], ss[:2], y[50:], cens[50:], HORIZONS))


@pytest.mark.parametrize("name,nh", [("bd3", 1), ("bd10", 5), ("ring5", 2), ("stiff6", 5)])
def test_host_function_is_the_restatement(lib, name, nh):
    S, s = CASES[name]()
    ages = np.array([1e-6, 1e-3, 0.1, 1.0, 5.0, 20.0])
    ages = ages[_mu(S) * ages <= EC.MU_Y_MAX]
    h = _hs(S)[:nh] if nh > 1 else np.array([0.7])
    Ss, ss = [S, 1.1 * S], [s, 1.1 * s]
    want = Sp.spares(Ss, ss, ages, _ones(len(ages)), h)
    assert not want["flags"].any() and not want["nbad"].any()
    st = None
    for d in range(2):
        st = P.spares_host(Ss[d], ss[d], ages, h, state=st)
        for k in ("words", "scales", "d", "var", "Delta", "V", "nbad", "nunits", "flags"):
            assert _bits(st[k][0]) == _bits(want[k][d]), (k, d)
    for k in ("dsum", "vsum", "d2sum", "cnt", "demand_unit", "demand_unit_sd"):
        assert _bits(st[k]) == _bits(want[k]), k
    # the words of two halves of the fleet add to the whole's (the table sized for the whole's largest age)
    ymax = float(np.max(ages))
    half = len(ages) // 2
    a = P.spares_host(S, s, ages[:half], h, ymax_c=ymax)
    b = P.spares_host(S, s, ages[half:], h, ymax_c=ymax)
    assert np.array_equal(a["words"] + b["words"], want["words"][:1]) and _bits(a["scales"]) == _bits(want["scales"][:1])


def test_host_function_refusals(lib):
    S, s = bd_exit(3)
    ok = np.array([1.0, 2.0])
    P.spares_host(S, s, ok, [0.5])
    with pytest.raises(P.PhaseTypeError, match="no censored unit"):
        P.spares_host(S, s, np.zeros(0), [0.5])
    for h in ([], np.arange(17.0), [-1.0], [np.nan], [1.0, np.inf], [1.0, 1.0], [2.0, 1.0]):
        with pytest.raises(P.PhaseTypeError, match="horizon"):
            P.spares_host(S, s, ok, h)
    with pytest.raises(P.PhaseTypeError, match="ymax_c"):
        P.spares_host(S, s, ok, [0.5], ymax_c=1.5)
    with pytest.raises(ValueError, match="state"):
        P.spares_host(S, s, ok, [0.5], state=P.spares_host(S, s, ok, [0.5, 1.0]))
    r = P.spares_host(S, s, ok, np.arange(16.0))
    assert r["d"].shape == (1, 2, 16) and r["words"].shape == (1, 34) and r["scales"].shape == (1, 32)


def test_exports(lib):
    names = ["pht_ctx_spares", "pht_ctx_spares_grid_cap", "pht_ctx_spares_ms", "pht_spares_host"]
    src = open(os.path.join(os.path.dirname(HERE), "include", "phasetype_amd.h")).read()
    for name in names:
        assert name in P.EXPORTS and hasattr(lib, name) and (name + "(") in src, name
    for name in ("fleet_spares", "spares_combine", "spares_finalise", "spares_host", "ph_renewal"):
        assert name in P.__all__ and hasattr(P, name), name
    assert hasattr(P.Sweeper, "spares")
    assert Sp.spec().sspec_nwords(16) == 34 and Sp.spec().sspec_q_r() > 0 and Sp.spec().sspec_v_r() > 0
