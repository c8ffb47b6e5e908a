"""GPU: the spares kernels (phasetype_amd/csrc/pht_spares.hip) against the tests'
restatement of include/pht_spares.h (tests/spares_spec.c), bit for bit in every
output: the words, the scales, the per-unit sums, cnt, the pointwise D / var
and the flags, in the caller's order; agreement with Sweeper.condition; mixed
table sizes; the bad and flagged paths; independence of the grid; no
interference with a chain, the WAIC state, the forecast or the condition;
fleet_spares end to end against the truth within the header's constants."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import condition_ref as Cd  # noqa: E402
import evaluator_cases as EC  # noqa: E402
import forecast_ref as F  # noqa: E402
import loglik_unif_ref as U  # noqa: E402
import phasetype_amd as P  # noqa: E402
import spares_ref as Sp  # noqa: E402
from phasetype_amd.synth import bd_exit, bd_exit_structure, simulate_ph  # noqa: E402

pytestmark = pytest.mark.gpu

ECS, UNIF = 2, 8
ULP = 2.0 ** -53
H1 = np.array([0.7])
H16 = np.concatenate([[0.0, 1e-9], np.geomspace(1e-3, 8.0, 14)])
HS = {1: H1, 16: H16}


def _gen(name):
    return U.ring(5) if name == "ring5" else bd_exit(int(name[2:]))


def _draws(S, s, nd):
    scales = np.linspace(0.8, 1.25, nd) if nd > 1 else np.array([1.0])
    return [S * c for c in scales], [s * c for c in scales]


def _fleet(units, seed=4):
    """``units`` censored observations with as many exact ones mixed in, in no
    order, ties among the ages and between an exact and a censored one
    (tests/test_gpu_condition.py's fleet, restated)"""
    rng = np.random.default_rng(seed + units)
    y = np.round(rng.exponential(3.0, 2 * units), 2) + 0.01
    cens = np.zeros(2 * units, np.int32)
    cens[rng.permutation(2 * units)[:units]] = 1
    if units > 2:
        i = np.flatnonzero(cens)
        y[i[1]] = y[i[0]]
        y[np.flatnonzero(cens == 0)[0]] = y[i[0]]
    return y, cens


def _run(n, y, cens, Ss, ss, h, batch=64, grid_cap=0, method=ECS, condition=False):
    sw = P.Sweeper(n, method, 1, device=0)
    try:
        sw.set_obs(y, cens)
        got = sw.spares(Ss, ss, h, batch=batch, pointwise=True, grid_cap=grid_cap)
        if condition:
            return got, sw.condition(Ss, ss, h, batch=batch, pointwise=True)
        return got
    finally:
        sw.close()


# censored units (1, 63, 64, 65: the wave's edges; 257, 1000: more than one
# block of 512, no multiple of it) x draws (1, 3, 65 with batch 64; 5 with
# batch 2: several batches, the sums in draw order across them) x H (1, 16)
# x generator (bd3, bd10, bd20, ring5: compile-time n; bd7, bd32: runtime n)
CASES = [(1, 1, 64, 1, "bd3"), (63, 3, 64, 16, "bd3"), (64, 65, 64, 1, "bd10"), (65, 5, 2, 16, "bd10"),
         (257, 3, 64, 16, "ring5"), (1000, 65, 64, 1, "bd10"), (1000, 5, 2, 1, "ring5"), (257, 1, 64, 16, "bd20"),
         (64, 3, 64, 1, "ring5"), (65, 65, 64, 16, "bd3"), (1000, 3, 64, 16, "bd3"), (1, 5, 2, 16, "ring5"),
         (257, 5, 2, 1, "bd3"), (257, 3, 64, 1, "bd7"), (65, 3, 64, 16, "bd32"), (63, 5, 2, 1, "bd20")]


@pytest.mark.parametrize("units,nd,batch,H,gen", CASES)
def test_bit_equal_to_the_restatement(gpu, units, nd, batch, H, gen):
    S, s = _gen(gen)
    n = S.shape[0]
    Ss, ss = _draws(S, s, nd)
    y, cens = _fleet(units)
    got = _run(n, y, cens, Ss, ss, HS[H], batch=batch)
    want = Sp.spares(Ss, ss, y, cens, HS[H])
    assert Sp.same_bits(got, want) == []
    assert got["d"].shape == (nd, units, H) and got["var"].shape == (nd, units, H)
    assert np.all(np.isfinite(got["d"])) and np.all(got["var"] >= 0) and np.all(np.isfinite(got["var"]))
    assert np.all(got["cnt"] == nd) and np.all(got["nunits"] == units) and not got["flags"].any()
    assert np.array_equal(got["unit_index"], np.flatnonzero(cens))
    if H == 16:  # h = 0: exact zeros
        assert not got["d"][:, :, 0].any() and not got["var"][:, :, 0].any() and not got["words"][:, [0, 16]].any()


@pytest.mark.parametrize("units,nd,batch,H,gen", [(257, 5, 2, 16, "bd10"), (65, 3, 64, 1, "bd7")])
def test_agrees_with_the_condition(gpu, units, nd, batch, H, gen):
    S, s = _gen(gen)
    n = S.shape[0]
    Ss, ss = _draws(S, s, nd)
    y, cens = _fleet(units)
    got, cond = _run(n, y, cens, Ss, ss, HS[H], batch=batch, condition=True)
    for k in ("d", "dsum", "Delta", "flags", "cnt", "nbad", "nunits", "demand_unit"):
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(cond[k]).tobytes(), k
    assert np.array_equal(got["words"][:, :H], cond["words"][:, n + 1:n + 1 + H])
    assert np.array_equal(got["scales"][:, :H], cond["scales"][:, 1:])


@pytest.fixture(scope="module")
def sweepers(gpu):
    """one context per n for the cases of evaluator_cases.OFF_BD_GPU"""
    held = {}

    def get(n):
        if n not in held:
            held[n] = P.Sweeper(n, ECS, 1, device=0)
        return held[n]

    yield get
    for sw in held.values():
        sw.close()


POINTS = Sp.POINT + ("Delta", "V", "demand_unit", "demand_unit_sd", "dsum", "vsum", "d2sum", "scales")
TRUTH_ON_GPU = ("hypoexp-10", "stiff-12")


def _clean(r):
    """no draw flagged, no unit bad, every value finite"""
    assert not r["flags"].any() and not r["bad_draw"].any() and not r["nbad"].any()
    for k in POINTS:
        assert np.all(np.isfinite(r[k])), k


def _var_within_contract(S, s, y, cens, h, d, var):
    """d, var [units, H] of the draw (S, s) against the truth at every distinct
    age, within the recorded constants on top of phi's contract and the dots'
    roundings (the tolerance of tests/test_spares.py's
    test_a_units_var_within_the_constants_and_phis_contract); the largest
    error / tolerance of var"""
    import mpmath as mp

    n, mu = S.shape[0], float(np.max(-np.diag(S)))
    _, ages = Sp.units(y, cens)
    first = np.unique(ages, return_index=True)[1]
    _, bad, khi = Cd.windows(S, s, ages[first], ymax_c=float(np.max(ages)))
    assert not bad.any()
    phi = Cd.truth_phi(S, ages[first])
    m1, m2 = Sp.truth_moments(S, s, h)
    worst = 0.0
    for i, u in enumerate(first):
        pb = [Cd.spec().cspec_phi_bound(n, int(khi[i]), float(phi[i][k])) for k in range(n)]
        for j, hj in enumerate(h):
            D = mp.fsum(p * a for p, a in zip(phi[i], m1[j]))
            Q = mp.fsum(p * a for p, a in zip(phi[i], m2[j]))
            vt = Q + D - D * D
            Df, Qf = float(D), float(Q)
            tol = Sp.spec().sspec_var_bound(mu * hj, Df, Qf) + (n + 2) * ULP * (Qf + Df + 2 * Df * Df) + \
                sum(pb[k] * float(m2[j][k] + m1[j][k] + 2 * D * m1[j][k]) for k in range(n))
            e = float(abs(mp.mpf(float(var[u, j])) - vt))
            assert e <= tol, (ages[u], hj, e, tol)
            if tol > 0:
                worst = max(worst, e / tol)
            assert abs(d[u, j] - Df) <= (Cd.spec().cspec_r_bound(mu * hj) + (n + 2) * ULP) * Df + \
                sum(pb[k] * float(m1[j][k]) for k in range(n)), (ages[u], hj)
    return worst


@pytest.mark.parametrize("case", EC.OFF_BD_GPU, ids=EC.case_id)
def test_off_bd_exit_bit_equal_to_the_restatement(gpu, sweepers, case):
    """The families of tests/evaluator_cases.py (single-successor rows, exact
    zeros in phi, a shift for R, rates over four decades) through the
    device-built r_h / q_h recurrences: 5 draws, 65 units among 130
    observations with ties, the horizons within the tables; batch 64 and 2;
    d is the condition's bit for bit.  On hypoexp10 and stiff12 the kernel's
    own var and d are held to the truth as well."""
    S, s, y, cens, h = EC.off_bd_case(case)
    n, H = S.shape[0], len(h)
    Ss, ss = U.scaled(S, s)
    want = Sp.spares(Ss, ss, y, cens, h)
    _clean(want)
    assert want["var"].shape == (5, 65, H) and np.all(want["cnt"] == 5) and np.all(want["nunits"] == 65)
    sw = sweepers(n)
    sw.set_obs(y, cens)
    for batch in (64, 2):
        got = sw.spares(Ss, ss, h, batch=batch, pointwise=True)
        _clean(got)
        assert Sp.same_bits(got, want) == [], batch
        assert np.all(got["var"] >= 0) and not got["d"][:, :, 0].any() and not got["var"][:, :, 0].any()  # h = 0
        cond = sw.condition(Ss, ss, h, batch=batch, pointwise=True)
        for k in ("d", "dsum", "Delta", "flags", "cnt", "nbad", "nunits", "demand_unit"):
            assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(cond[k]).tobytes(), (k, batch)
        assert np.array_equal(got["words"][:, :H], cond["words"][:, n + 1:n + 1 + H])
        assert np.array_equal(got["scales"][:, :H], cond["scales"][:, 1:])
    if EC.case_id(case) in TRUTH_ON_GPU:
        worst = _var_within_contract(Ss[2], ss[2], y, cens, h, got["d"][2], got["var"][2])
        print(f"{EC.case_id(case)}: the kernel's var, largest error / tolerance {worst:.4f}")


def test_table_sizes_mixed_in_one_batch(gpu):
    """the renewal side: mu h_max = 1440 for two of the draws (Kr just below
    the cap) and about 10 for the rest; the (ax, ac) side: mu ymax_c = 1480 for
    two of the draws, K = 2047, one table an LDS pass, the others share passes"""
    S, s = bd_exit(3)
    y, cens = _fleet(130)
    ymax = float(np.max(y[cens != 0]))
    mu0 = float(np.max(-np.diag(S)))
    # the renewal side
    hmax = 2.0
    big, small = 1440.0 / (mu0 * hmax), 10.0 / (mu0 * hmax)
    scales = [small, 1.2 * small, big, 0.9 * small, 0.999 * big, 1.1 * small, small]
    Ss, ss = [S * c for c in scales], [s * c for c in scales]
    h = np.array([0.01, 0.5, hmax])
    want = Sp.spares(Ss, ss, y, cens, h)
    Krs = [Sp.vectors(A, b, h)[3] for A, b in zip(Ss, ss)]
    assert 2000 < Krs[2] < 2047 and 2000 < Krs[4] < 2047 and max(Krs[0], Krs[1], Krs[3]) < 150, Krs
    assert not want["flags"].any()
    got = _run(3, y, cens, Ss, ss, h)
    assert Sp.same_bits(got, want) == []
    print("renewal side, bad units per draw:", got["nbad"].tolist())
    # the (ax, ac) side
    big, small = 1480.0 / (mu0 * ymax), 10.0 / (mu0 * ymax)
    scales = [small, 1.2 * small, big, 0.9 * small, 0.99 * big, 1.1 * small, small]
    Ss, ss = [S * c for c in scales], [s * c for c in scales]
    Ks = [U.table(A, b, ymax)["K"] for A, b in zip(Ss, ss)]
    assert Ks[2] == 2047 and Ks[4] == 2047 and 100 < max(Ks[0], Ks[1], Ks[3]) < 150, Ks
    h = np.array([0.5, 8.0]) / big  # mu h stays far below the renewal table's cap for every draw
    got = _run(3, y, cens, Ss, ss, h)
    want = Sp.spares(Ss, ss, y, cens, h)
    assert Sp.same_bits(got, want) == []
    print("table side, bad units per draw:", got["nbad"].tolist())
    assert not got["flags"].any() and got["nbad"][0] == 0


def test_flagged_draws_mid_batch_and_bad_units(gpu):
    S, s = bd_exit(3)
    Sn = S.copy()
    Sn[2, 1] = np.nan
    trap, st = S.copy(), s.copy()  # state 3 neither moves nor exits
    trap[2, :] = 0.0
    st[2] = 0.0
    mu = float(np.max(-np.diag(S)))
    # draw 5 alone has mu h_max beyond the renewal table's sizing rule
    Ss, ss = [S, 0.9 * S, Sn, 1.1 * S, trap, 4.0 * S, 1.2 * S], [s, 0.9 * s, s, 1.1 * s, st, 4.0 * s, 1.2 * s]
    y, cens = _fleet(65)
    h = np.array([1.0, 500.0 / mu])
    got, cond = _run(3, y, cens, Ss, ss, h, condition=True)
    want = Sp.spares(Ss, ss, y, cens, h)
    assert Sp.same_bits(got, want) == []
    assert got["flags"].tolist() == [0, 0, 4, 0, 64, 128, 0] and np.array_equal(got["flags"], cond["flags"])
    for d in (2, 4, 5):
        assert not got["words"][d].any() and not got["scales"][d].any()
        assert np.all(np.isnan(got["d"][d])) and np.all(np.isnan(got["var"][d]))
    assert np.all(got["cnt"] == 4) and got["nunits"].tolist() == [65, 65, 0, 65, 0, 0, 65]
    # units at mu c = 3000 lie beyond every table: bad in every draw, counted and never summed
    S, s = bd_exit(5)
    Ss, ss = _draws(S, s, 3)
    y, cens = _fleet(130)
    mu = float(np.max(-np.diag(Ss[0])))
    far = np.flatnonzero(cens)[[3, 77]]
    y[far] = 3000.0 / mu
    got = _run(5, y, cens, Ss, ss, H1)
    want = Sp.spares(Ss, ss, y, cens, H1)
    assert Sp.same_bits(got, want) == []
    rows = np.flatnonzero(np.isin(got["unit_index"], far))
    assert got["nbad"].tolist() == [2, 2, 2] and got["nunits"].tolist() == [128] * 3
    assert np.all(got["cnt"][rows] == 0) and np.all(np.delete(got["cnt"], rows) == 3)
    assert np.all(np.isnan(got["var"][:, rows])) and np.all(np.isnan(got["demand_unit_sd"][rows]))
    assert not got["dsum"][rows].any() and not got["vsum"][rows].any() and not got["d2sum"][rows].any()


def test_callers_order_and_grid_independence(gpu):
    S, s = bd_exit(10)
    Ss, ss = _draws(S, s, 3)
    y, cens = _fleet(1000)
    base = _run(10, y, cens, Ss, ss, H16)
    for cap in (1, 3):
        assert Sp.same_bits(_run(10, y, cens, Ss, ss, H16, grid_cap=cap), base) == []
    perm = np.random.default_rng(1).permutation(len(y))
    got = _run(10, y[perm], cens[perm], Ss, ss, H16)
    assert np.array_equal(got["words"], base["words"]) and np.array_equal(got["scales"], base["scales"])
    # unit r of the shuffled call is observation perm[unit_index[r]] of the first
    where = {int(i): r for r, i in enumerate(base["unit_index"])}
    rows = np.array([where[int(perm[i])] for i in got["unit_index"]])
    for k in ("dsum", "vsum", "d2sum", "cnt", "demand_unit", "demand_unit_sd"):
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(base[k][rows]).tobytes(), k
    for k in Sp.POINT:
        assert got[k].tobytes() == np.ascontiguousarray(base[k][:, rows]).tobytes(), k
    # a DCS context keeps exact and censored observations in one sorted range
    assert Sp.same_bits(_run(10, y, cens, Ss, ss, H16, method=4), base) == []


def test_refusals(gpu):
    S, s = bd_exit(3)
    sw = P.Sweeper(3, ECS, 1, device=0)
    try:
        with pytest.raises(P.PhaseTypeError, match="no censored observation"):
            sw.spares([S], [s], [1.0])
        sw.set_obs(np.array([1.0, 2.0]), np.zeros(2, np.int32))
        with pytest.raises(P.PhaseTypeError, match="no censored observation"):
            sw.spares([S], [s], [1.0])
        sw.set_obs(np.array([1.0, 2.0, 3.0]), np.array([0, 1, 1], np.int32))
        for h in ([], np.arange(17.0), [-1.0], [np.nan], [1.0, np.inf], [1.0, 1.0], [2.0, 1.0]):
            with pytest.raises(P.PhaseTypeError, match="horizon"):
                sw.spares([S], [s], h)
        for batch in (0, 65):
            with pytest.raises(P.PhaseTypeError, match="batch"):
                sw.spares([S], [s], [1.0], batch=batch)
        r = sw.spares([S], [s], [1.0])
        assert r["nunits"].tolist() == [2] and "d" not in r and len(sw.last_spares_ms) == 2
        assert r["unit_index"].tolist() == [1, 2] and r["V"].shape == (1, 1)
    finally:
        sw.close()


def test_ph_renewal_is_one_unit_of_the_restatement(gpu):
    S, s = bd_exit(3)
    h = np.array([[0.0, 0.5], [2.0, 7.0]])
    want = Sp.spares([S], [s], [1.5], [1], h.reshape(-1))
    m, v = P.ph_renewal(S, s, h, given=1.5)
    assert m.shape == (2, 2) and m.tobytes() == want["d"][0, 0].tobytes() and v.tobytes() == want["var"][0, 0].tobytes()
    m0, v0 = P.ph_renewal(S, s, 2.0)  # a new unit, one horizon: two floats
    new = Sp.spares([S], [s], [0.0], [1], [2.0])
    assert isinstance(m0, float) and isinstance(v0, float) and (m0, v0) == (new["d"][0, 0, 0], new["var"][0, 0, 0])
    trap, st = S.copy(), s.copy()
    trap[2, :] = 0.0
    st[2] = 0.0
    with pytest.raises(ValueError, match="flag 64"):
        P.ph_renewal(trap, st, 1.0)


def test_chain_waic_forecast_and_condition_are_untouched(gpu):
    n, it = 3, 6
    T = np.zeros((4, 4), np.int32)
    T[0, 1], T[0, 3], T[1, 2], T[1, 3], T[2, 0], T[2, 3] = 1, 2, 3, 4, 5, 6
    theta = np.array([1.0, 0.1, 1.0, 0.1, 1.0, 0.1])
    S, s = P.theta_to_S(theta, T)
    y, cen = simulate_ph(S, s, 1000, seed=15, censor_frac=0.3)
    nu, zeta, Cm, zexp = 1 + 50 * theta, np.full(len(theta), 50.0), np.ones(T.shape), P.zexp_for(y)

    def run(with_s):
        P.set_seed(1)
        sw = P.Sweeper(n, UNIF, 1, device=0)
        sw.set_obs(y, cen)
        sw.waic_reset()
        if with_s:
            sw.spares([S, 1.1 * S], [s, 1.1 * s], H16)
        a = sw.loglik_unif([S, 1.1 * S], [s, 1.1 * s], accumulate=True)
        if with_s:
            sw.spares([S], [s], H1, batch=1, pointwise=True)
        f1 = sw.forecast([S, 1.1 * S], [s, 1.1 * s], H16, pointwise=True)
        k1 = sw.condition([S, 1.1 * S], [s, 1.1 * s], H16, pointwise=True)
        c1 = sw.gibbs(it, UNIF, nu, zeta, T, Cm, zexp)
        if with_s:
            sw.spares([0.9 * S] * 65, [0.9 * s] * 65, [0.5, 40.0])
        b = sw.loglik_unif([0.9 * S], [0.9 * s], accumulate=True)
        f2 = sw.forecast([0.9 * S], [0.9 * s], H1)
        k2 = sw.condition([0.9 * S], [0.9 * s], H1)
        c2 = sw.gibbs(it, UNIF, nu, zeta, T, Cm, zexp, start=c1[-1])
        st = sw.waic_state()
        sw.close()
        return a, b, st, np.concatenate([c1, c2]), f1, f2, k1, k2

    wa, wb, wst, wc, wf1, wf2, wk1, wk2 = run(True)
    a, b, st, c, f1, f2, k1, k2 = run(False)
    for k in ("H", "F", "nbad", "nobs"):
        assert np.array_equal(wa[k], a[k]) and np.array_equal(wb[k], b[k]), k
    for k in ("ref", "S1", "S2", "m", "r"):
        assert np.ascontiguousarray(wst[k]).tobytes() == np.ascontiguousarray(st[k]).tobytes(), k
    assert np.array_equal(wst["cnt"], st["cnt"])
    assert wc.tobytes() == c.tobytes()
    assert F.same_bits(wf1, f1) == [] and F.same_bits(wf2, f2) == []
    assert Cd.same_bits(wk1, k1) == [] and Cd.same_bits(wk2, k2) == []


def test_fleet_spares_at_size_within_the_constants(gpu):
    """n = 10, 2000 units, 64 draws through the public function; the chain
    alternates between two parameter vectors.  var of 5 units x 3 horizons of
    each of the two draws against the truth: the recorded bound, the n + 2
    roundings of each dot and what phi's contract allows
    (tests/test_spares.py's unit bound).  The values come from
    ``Sweeper.spares`` pointwise on the same fleet, whose words fleet_spares'
    are."""
    import mpmath as mp

    n = 10
    T, theta = bd_exit_structure(n)
    S0, s0 = P.theta_to_S(theta, T)
    x, _ = simulate_ph(S0, s0, 2000, seed=33, censor_frac=0.0)
    cen = np.ones(2000, np.int32)
    res = np.stack([theta, 1.1 * theta] * 32)
    h = np.array([0.1, 1.0, 10.0])
    draws = [P.theta_to_S(theta, T), P.theta_to_S(1.1 * theta, T)]
    Ss, ss = [d[0] for d in draws], [d[1] for d in draws]
    # the inputs: the restatement itself has no bad unit and no flagged draw
    spec = Sp.spares(Ss, ss, x, cen, h)
    assert not spec["flags"].any() and not spec["nbad"].any() and np.all(spec["nunits"] == 2000)
    out = P.fleet_spares(res, x, T, h, cen)
    cond = P.fleet_condition(res, x, T, cen, h)
    assert out["n_used"].tolist() == [64] * 3 and not out["nbad"].any() and np.all(out["cnt"] == 64)
    assert out["demand_unit"].shape == (2000, 3) and out["demand_unit_sd"].shape == (2000, 3)
    # the draws' words are the restatement's, draw for draw
    assert np.array_equal(out["words"][0], spec["words"][0]) and np.array_equal(out["words"][1], spec["words"][1])
    assert np.array_equal(out["words"][62], spec["words"][0]) and np.array_equal(out["words"][63], spec["words"][1])
    # the law of total variance, and its two parts
    # (sd is the rounded root: its square is the sum to 3 roundings)
    assert np.allclose(out["sd"] ** 2, out["within"] + out["between"], rtol=4 * ULP, atol=0)
    assert np.array_equal(out["Delta"], cond["Delta"]) and np.array_equal(out["mean"], cond["demand_mean"])
    assert np.allclose(out["between"], cond["demand_sd"] ** 2, rtol=1e-12, atol=0)
    assert np.all(out["within"] > 0) and np.all(out["sd"] >= cond["demand_sd"]) and np.all(out["sd"] > cond["demand_sd"])
    stock = out["stock"](0.95)
    assert stock.shape == (1, 3) and np.all(stock == np.floor(stock)) and np.all(stock[0] >= out["mean"])
    assert np.all(out["stock"](0.5)[0] <= stock[0])
    # the per-unit sd: within + between over the two alternating draws
    want_sd = np.sqrt(spec["var"].mean(0) + spec["d"].var(0))
    assert np.allclose(out["demand_unit_sd"], want_sd, rtol=1e-10, atol=0)
    # 5 units x 3 horizons x 2 draws against the truth
    pick = np.argsort(x)[np.linspace(0, 1999, 5).astype(int)]
    ymax_c = float(np.max(x))
    sw = P.Sweeper(n, ECS, 1, device=0)
    try:
        sw.set_obs(x, cen)
        pw = sw.spares(Ss, ss, h, pointwise=True)
    finally:
        sw.close()
    assert np.array_equal(pw["words"], out["words"][:2])
    worst = 0.0
    for d, (S, s) in enumerate(draws):
        mu = float(np.max(-np.diag(S)))
        phi = Cd.truth_phi(S, x[pick])
        _, bad, khi = Cd.windows(S, s, x[pick], ymax_c=ymax_c)
        assert not bad.any()
        m1, m2 = Sp.truth_moments(S, s, h)
        for i in range(5):
            for j, hj in enumerate(h):
                D = mp.fsum(p * a for p, a in zip(phi[i], m1[j]))
                Q = mp.fsum(p * a for p, a in zip(phi[i], m2[j]))
                Df, Qf = float(D), float(Q)
                tol = Sp.spec().sspec_var_bound(mu * hj, Df, Qf) + (n + 2) * ULP * (Qf + Df + 2 * Df * Df) + \
                    sum(Cd.spec().cspec_phi_bound(n, int(khi[i]), float(phi[i][k]))
                        * float(m2[j][k] + m1[j][k] + 2 * D * m1[j][k]) for k in range(n))
                e = float(abs(mp.mpf(float(pw["var"][d, pick[i], j])) - (Q + D - D * D)))
                worst = max(worst, e / tol)
                assert e <= tol, (d, i, hj, e, tol)
    print(f"largest error / bound {worst:.3f}")
