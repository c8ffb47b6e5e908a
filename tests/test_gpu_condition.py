"""GPU: the condition kernels (phasetype_amd/csrc/pht_condition.hip) against the
tests' restatement of include/pht_condition.h (tests/condition_spec.c), bit for
bit in every output: the words, the scales, the per-unit sums, cnt, the
pointwise phi / MRL / D and the flags, in the caller's order; the bad and
flagged paths; independence of the grid; no interference with a chain, the WAIC
state or the forecast; fleet_condition end to end against the truth within the
header's contract."""
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
from phasetype_amd.synth import bd_exit, bd_exit_structure, simulate_ph  # noqa: E402

pytestmark = pytest.mark.gpu

ECS, UNIF = 2, 8
H1 = np.array([0.7])
H16 = np.concatenate([[0.0, 1e-9], np.geomspace(1e-3, 8.0, 14)])
HS = {0: None, 1: H1, 16: H16}
ALL = Cd.KEYS + Cd.POINT + Cd.DERIVED


def _gen(name):
    return U.ring(5) if name == "ring5" else bd_exit(int(name[2:]))


def _draws(S, s, nd):
    scales = np.linspace(0.8, 1.25, nd) if nd > 1 else np.array([1.0])
    return [S * c for c in scales], [s * c for c in scales]


def _fleet(units, seed=4):
    """``units`` censored observations with as many exact ones mixed in, in no
    order, ties among the ages and between an exact and a censored one
    (tests/test_gpu_forecast.py's fleet, restated)"""
    rng = np.random.default_rng(seed + units)
    y = np.round(rng.exponential(3.0, 2 * units), 2) + 0.01
    cens = np.zeros(2 * units, np.int32)
    cens[rng.permutation(2 * units)[:units]] = 1
    if units > 2:
        i = np.flatnonzero(cens)
        y[i[1]] = y[i[0]]
        y[np.flatnonzero(cens == 0)[0]] = y[i[0]]
    return y, cens


def _run(n, y, cens, Ss, ss, h, batch=64, grid_cap=0, method=ECS):
    sw = P.Sweeper(n, method, 1, device=0)
    try:
        sw.set_obs(y, cens)
        return sw.condition(Ss, ss, h, batch=batch, pointwise=True, grid_cap=grid_cap)
    finally:
        sw.close()


# censored units (1, 63, 64, 65: the wave's edges; 257, 1000: more than one
# block of 512, no multiple of it) x draws (1, 3, 65 with batch 64; 5 with
# batch 2: several batches, the sums in draw order across them) x H (0, 1, 16)
# x generator (bd3, bd10, bd20, ring5: compile-time n; bd7, bd32: runtime n)
CASES = [(1, 1, 64, 0, "bd3"), (63, 3, 64, 16, "bd3"), (64, 65, 64, 1, "bd10"), (65, 5, 2, 16, "bd10"),
         (257, 3, 64, 16, "ring5"), (1000, 65, 64, 1, "bd10"), (1000, 5, 2, 0, "ring5"), (257, 1, 64, 16, "bd20"),
         (64, 3, 64, 0, "ring5"), (65, 65, 64, 16, "bd3"), (1000, 3, 64, 16, "bd3"), (1, 5, 2, 1, "ring5"),
         (63, 65, 64, 0, "bd10"), (257, 5, 2, 1, "bd3"), (257, 3, 64, 1, "bd7"), (65, 3, 64, 16, "bd32"),
         (1000, 3, 64, 16, "bd10"), (65, 5, 2, 0, "bd20")]


@pytest.mark.parametrize("units,nd,batch,H,gen", CASES)
def test_bit_equal_to_the_restatement(gpu, units, nd, batch, H, gen):
    S, s = _gen(gen)
    n = S.shape[0]
    Ss, ss = _draws(S, s, nd)
    y, cens = _fleet(units)
    got = _run(n, y, cens, Ss, ss, HS[H], batch=batch)
    want = Cd.condition(Ss, ss, y, cens, HS[H])
    assert Cd.same_bits(got, want, ALL) == []
    assert got["phi"].shape == (nd, units, n) and got["d"].shape == (nd, units, H)
    assert np.all(np.isfinite(got["phi"])) and np.all(np.isfinite(got["mrl"])) and np.all(np.isfinite(got["d"]))
    assert np.all(got["cnt"] == nd) and np.all(got["nunits"] == units) and not got["flags"].any()
    assert np.array_equal(got["unit_index"], np.flatnonzero(cens))


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


def _clean(r):
    """no draw flagged, no unit bad, every value finite"""
    assert not r["flags"].any() and not r["bad_draw"].any() and not r["nbad"].any()
    for k in POINTS:
        assert np.all(np.isfinite(r[k])), k


POINTS = Cd.POINT + ("Phi", "L", "Delta", "p_phase", "mrl_unit", "demand_unit", "phisum", "mrlsum", "dsum", "scales")
TRUTH_ON_GPU = ("hypoexp-10", "stiff-12")


def _phi_within_contract(S, s, y, cens, phi):
    """phi [units, n] of the draw (S, s) against the truth at every distinct
    age, within the header's contract (as tests/test_condition.py holds the
    restatement to it); the largest error / bound"""
    import mpmath as mp

    n = S.shape[0]
    _, ages = Cd.units(y, cens)
    first = np.unique(ages, return_index=True)[1]
    _, bad, khi = Cd.windows(S, s, ages[first], ymax_c=float(np.max(ages)))
    assert not bad.any()
    truth = Cd.truth_phi(S, ages[first])
    worst = 0.0
    for i, u in enumerate(first):
        for j in range(n):
            b = Cd.spec().cspec_phi_bound(n, int(khi[i]), float(truth[i][j]))
            e = float(abs(mp.mpf(float(phi[u, j])) - truth[i][j]))
            worst = max(worst, e / b)
            assert e <= b, (ages[u], j, e, b)
    return worst


@pytest.mark.parametrize("case", EC.OFF_BD_GPU, ids=EC.case_id)
def test_off_bd_exit_bit_equal_to_the_restatement(gpu, sweepers, case):
    """The families of tests/evaluator_cases.py: single-successor rows, exact
    zeros in the forward vectors and in phi, a shift for R (Erlang), rates over
    four decades (stiff); 5 draws, 65 units among 130 observations with ties,
    the horizons within the tables; batch 64 and 2.  On hypoexp10 and stiff12
    the kernel's own phi is held to the truth as well."""
    S, s, y, cens, h = EC.off_bd_case(case)
    n = S.shape[0]
    Ss, ss = U.scaled(S, s)
    want = Cd.condition(Ss, ss, y, cens, h)
    _clean(want)
    assert want["phi"].shape == (5, 65, n) and np.all(want["cnt"] == 5) and np.all(want["nunits"] == 65)
    sw = sweepers(n)
    sw.set_obs(y, cens)
    for batch in (64, 2):
        got = sw.condition(Ss, ss, h, batch=batch, pointwise=True)
        _clean(got)
        assert Cd.same_bits(got, want, ALL) == [], batch
    print(f"{EC.case_id(case)}: exact zeros in phi {int((got['phi'] == 0).sum())} of {got['phi'].size}")
    if EC.case_id(case) in TRUTH_ON_GPU:
        worst = _phi_within_contract(Ss[2], ss[2], y, cens, got["phi"][2])
        print(f"{EC.case_id(case)}: the kernel's phi, largest error / bound {worst:.4f}")


def test_table_sizes_mixed_in_one_call(gpu):
    """mu ymax_c = 1480 and 1465 for two of the draws (from 1457 on the sizing
    rule reaches the cap): K = 2047, one (ax, ac) table an LDS pass; the others
    have K about 120 (mu ymax_c = 9 .. 12) and share passes"""
    S, s = bd_exit(3)
    y, cens = _fleet(130)
    ymax = float(np.max(y[cens != 0]))
    mu0 = float(np.max(-np.diag(S)))
    big, small = 1480.0 / (mu0 * ymax), 10.0 / (mu0 * ymax)
    scales = [small, 1.2 * small, big, 0.9 * small, 0.99 * big, 1.1 * small, small]
    Ss, ss = [S * c for c in scales], [s * c for c in scales]
    Ks = [U.table(A, b, ymax)["K"] for A, b in zip(Ss, ss)]
    assert Ks[2] == 2047 and Ks[4] == 2047 and 100 < max(Ks[0], Ks[1], Ks[3]) < 150, Ks
    h = np.array([0.5, 8.0]) / big  # mu h stays far below the renewal table's cap for every draw
    got = _run(3, y, cens, Ss, ss, h)
    want = Cd.condition(Ss, ss, y, cens, h)
    assert Cd.same_bits(got, want, ALL) == []
    print("bad units per draw:", got["nbad"].tolist())
    assert not got["flags"].any() and got["nbad"][0] == 0


def test_flagged_draws_mid_batch_and_bad_units(gpu):
    S, s = bd_exit(3)
    Sn = S.copy()
    Sn[2, 1] = np.nan
    trap, st = S.copy(), s.copy()  # state 3 neither moves nor exits
    trap[2, :] = 0.0
    st[2] = 0.0
    Ss, ss = [S, 0.9 * S, Sn, 1.1 * S, trap, 1.2 * S], [s, 0.9 * s, s, 1.1 * s, st, 1.2 * s]
    y, cens = _fleet(65)
    h = np.array([1.0, 5.0])
    got = _run(3, y, cens, Ss, ss, h)
    want = Cd.condition(Ss, ss, y, cens, h)
    assert Cd.same_bits(got, want, ALL) == []
    assert got["flags"].tolist() == [0, 0, 4, 0, 64, 0]
    for d in (2, 4):
        assert not got["words"][d].any() and not got["scales"][d].any()
        assert np.all(np.isnan(got["phi"][d])) and np.all(np.isnan(got["mrl"][d])) and np.all(np.isnan(got["d"][d]))
    assert np.all(got["cnt"] == 4) and got["nunits"].tolist() == [65, 65, 0, 65, 0, 65]
    # a horizon beyond the renewal table flags the draw as a whole
    mu = float(np.max(-np.diag(S)))
    got = _run(3, y, cens, [S, 0.5 * S], [s, 0.5 * s], [1.0, 1600.0 / mu])
    want = Cd.condition([S, 0.5 * S], [s, 0.5 * s], y, cens, [1.0, 1600.0 / mu])
    assert Cd.same_bits(got, want, ALL) == [] and got["flags"].tolist() == [128, 0] and np.all(got["cnt"] == 1)


def test_units_bad_at_the_largest_age_only(gpu):
    """mu c = 3000 lies beyond every table: those units are bad in every draw,
    counted and never summed, and the others are untouched by them"""
    S, s = bd_exit(5)
    Ss, ss = _draws(S, s, 3)
    y, cens = _fleet(130)
    mu = float(np.max(-np.diag(Ss[0])))
    far = np.flatnonzero(cens)[[3, 77]]
    y[far] = 3000.0 / mu
    got = _run(5, y, cens, Ss, ss, H1)
    want = Cd.condition(Ss, ss, y, cens, H1)
    assert Cd.same_bits(got, want, ALL) == []
    rows = np.flatnonzero(np.isin(got["unit_index"], far))
    assert got["nbad"].tolist() == [2, 2, 2] and got["nunits"].tolist() == [128] * 3
    assert np.all(got["cnt"][rows] == 0) and np.all(np.delete(got["cnt"], rows) == 3)
    assert np.all(np.isnan(got["phi"][:, rows])) and np.all(np.isnan(got["p_phase"][rows]))
    assert not got["phisum"][rows].any() and not got["dsum"][rows].any()


def test_callers_order_and_grid_independence(gpu):
    S, s = bd_exit(10)
    Ss, ss = _draws(S, s, 3)
    y, cens = _fleet(1000)
    base = _run(10, y, cens, Ss, ss, H16)
    for cap in (1, 3):
        assert Cd.same_bits(_run(10, y, cens, Ss, ss, H16, grid_cap=cap), base, ALL) == []
    perm = np.random.default_rng(1).permutation(len(y))
    got = _run(10, y[perm], cens[perm], Ss, ss, H16)
    assert np.array_equal(got["words"], base["words"]) and np.array_equal(got["scales"], base["scales"])
    # unit r of the shuffled call is observation perm[unit_index[r]] of the first
    where = {int(i): r for r, i in enumerate(base["unit_index"])}
    rows = np.array([where[int(perm[i])] for i in got["unit_index"]])
    for k in ("phisum", "mrlsum", "dsum", "cnt", "p_phase", "mrl_unit", "demand_unit"):
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(base[k][rows]).tobytes(), k
    for k in Cd.POINT:
        assert got[k].tobytes() == np.ascontiguousarray(base[k][:, rows]).tobytes(), k
    # a DCS context keeps exact and censored observations in one sorted range
    assert Cd.same_bits(_run(10, y, cens, Ss, ss, H16, method=4), base, ALL) == []


def test_refusals(gpu):
    S, s = bd_exit(3)
    sw = P.Sweeper(3, ECS, 1, device=0)
    try:
        with pytest.raises(P.PhaseTypeError, match="no censored observation"):
            sw.condition([S], [s], [1.0])
        sw.set_obs(np.array([1.0, 2.0]), np.zeros(2, np.int32))
        with pytest.raises(P.PhaseTypeError, match="no censored observation"):
            sw.condition([S], [s])
        sw.set_obs(np.array([1.0, 2.0, 3.0]), np.array([0, 1, 1], np.int32))
        for h in (np.arange(17.0), [-1.0], [np.nan], [1.0, np.inf], [1.0, 1.0], [2.0, 1.0]):
            with pytest.raises(P.PhaseTypeError, match="horizon"):
                sw.condition([S], [s], h)
        for batch in (0, 65):
            with pytest.raises(P.PhaseTypeError, match="batch"):
                sw.condition([S], [s], [1.0], batch=batch)
        r = sw.condition([S], [s])
        assert r["nunits"].tolist() == [2] and "phi" not in r and len(sw.last_condition_ms) == 2
        assert r["unit_index"].tolist() == [1, 2] and r["Delta"].shape == (1, 0)
    finally:
        sw.close()


def test_waic_totals_forecast_and_chain_are_untouched(gpu):
    n, it = 3, 6
    T = np.zeros((4, 4), np.int32)
    T[0, 1], T[0, 3], T[1, 2], T[1, 3], T[2, 0], T[2, 3] = 1, 2, 3, 4, 5, 6
    theta = np.array([1.0, 0.1, 1.0, 0.1, 1.0, 0.1])
    S, s = P.theta_to_S(theta, T)
    y, cen = simulate_ph(S, s, 1000, seed=15, censor_frac=0.3)
    nu, zeta, Cm, zexp = 1 + 50 * theta, np.full(len(theta), 50.0), np.ones(T.shape), P.zexp_for(y)

    def run(with_c):
        P.set_seed(1)
        sw = P.Sweeper(n, UNIF, 1, device=0)
        sw.set_obs(y, cen)
        sw.waic_reset()
        if with_c:
            sw.condition([S, 1.1 * S], [s, 1.1 * s], H16)
        a = sw.loglik_unif([S, 1.1 * S], [s, 1.1 * s], accumulate=True)
        if with_c:
            sw.condition([S], [s], H1, batch=1, pointwise=True)
        f1 = sw.forecast([S, 1.1 * S], [s, 1.1 * s], H16, pointwise=True)
        c1 = sw.gibbs(it, UNIF, nu, zeta, T, Cm, zexp)
        if with_c:
            sw.condition([0.9 * S] * 65, [0.9 * s] * 65, [0.5, 40.0])
        b = sw.loglik_unif([0.9 * S], [0.9 * s], accumulate=True)
        f2 = sw.forecast([0.9 * S], [0.9 * s], H1)
        c2 = sw.gibbs(it, UNIF, nu, zeta, T, Cm, zexp, start=c1[-1])
        st = sw.waic_state()
        sw.close()
        return a, b, st, np.concatenate([c1, c2]), f1, f2

    wa, wb, wst, wc, wf1, wf2 = run(True)
    a, b, st, c, f1, f2 = run(False)
    for k in ("H", "F", "nbad", "nobs"):
        assert np.array_equal(wa[k], a[k]) and np.array_equal(wb[k], b[k]), k
    for k in ("ref", "S1", "S2", "m", "r"):
        assert np.ascontiguousarray(wst[k]).tobytes() == np.ascontiguousarray(st[k]).tobytes(), k
    assert np.array_equal(wst["cnt"], st["cnt"])
    assert wc.tobytes() == c.tobytes()
    assert F.same_bits(wf1, f1) == [] and F.same_bits(wf2, f2) == []


def test_fleet_condition_at_size_within_contract(gpu):
    """n = 10, 2000 units, 64 draws through the public function.  The chain
    alternates between two parameter vectors, so p_phase is the mean of two
    values of phi, each summed 32 times: the truth is the mean of the two
    truths, the bound the mean of the two contracts plus the rounding of the 63
    additions and the division (each at most 2^-53 of the final sum).  5 units
    x 10 phases = 50 cells."""
    n = 10
    T, theta = bd_exit_structure(n)
    S0, s0 = P.theta_to_S(theta, T)
    x, _ = simulate_ph(S0, s0, 2000, seed=33, censor_frac=0.0)
    cen = np.ones(2000, np.int32)
    res = np.stack([theta, 1.1 * theta] * 32)
    h = np.array([0.1, 1.0, 10.0])
    draws = [P.theta_to_S(theta, T), P.theta_to_S(1.1 * theta, T)]
    # the inputs: the restatement itself has no bad unit and no flagged draw
    spec = Cd.condition([d[0] for d in draws], [d[1] for d in draws], x, cen, h, pointwise=False)
    assert not spec["flags"].any() and not spec["nbad"].any() and np.all(spec["nunits"] == 2000)
    out = P.fleet_condition(res, x, T, cen, h)
    assert out["p_phase"].shape == (2000, n) and out["n_used"] == 64 and not out["nbad"].any()
    assert np.all(out["cnt"] == 64) and out["demand_unit"].shape == (2000, 3) and out["stage"].shape == (2000,)
    assert np.array_equal(out["stage"], np.argmax(out["p_phase"], axis=1))
    # the draws' words are the restatement's, draw for draw
    assert np.array_equal(out["words"][0], spec["words"][0]) and np.array_equal(out["words"][1], spec["words"][1])
    assert np.array_equal(out["words"][62], spec["words"][0])
    # the summaries are the words'
    assert np.allclose(out["phase"].sum(1), 2000.0, rtol=0, atol=1e-8)  # (20000 roundings to 2^-40)
    assert np.allclose(out["phase_mean"], out["p_phase"].sum(0), rtol=1e-9, atol=1e-8)
    assert np.allclose(out["residual_life_mean"], out["mrl_unit"].sum(), rtol=1e-9)
    assert np.allclose(out["demand_mean"], out["demand_unit"].sum(0), rtol=1e-9)
    assert np.all(np.diff(out["demand_mean"]) > 0) and np.all(out["demand_sd"] > 0)
    assert np.all(out["demand_band"][0] <= out["demand_mean"]) and np.all(out["demand_mean"] <= out["demand_band"][2])
    # 5 units x 10 phases against the truth
    pick = np.argsort(x)[np.linspace(0, 1999, 5).astype(int)]
    ymax_c = float(np.max(x))
    truth, bound = [], []
    for S, s in draws:
        t = np.array([[float(v) for v in row] for row in Cd.truth_phi(S, x[pick])])
        _, bad, khi = Cd.windows(S, s, x[pick], ymax_c=ymax_c)
        assert not bad.any()
        truth.append(t)
        bound.append(Cd.phi_bound(n, khi, t))
    want = 0.5 * (truth[0] + truth[1])
    tol = 0.5 * (bound[0] + bound[1]) + 64 * 2.0 ** -53 * want
    err = np.abs(out["p_phase"][pick] - want)
    print(f"largest error / bound {np.max(err / tol):.3f}")
    assert err.shape == (5, 10) and np.all(err <= tol), (err, tol)
