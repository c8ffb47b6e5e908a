"""GPU: the forecast kernel (phasetype_amd/csrc/pht_forecast.hip) against the
tests' restatement of include/pht_forecast.h (tests/forecast_spec.c), bit for
bit in every output: the words, qsum, cnt, the pointwise q and the flags, in
the caller's order; the bad and flagged paths; independence of the grid; no
interference with a chain or the WAIC state; fleet_forecast end to end against
the truth within the header's contract."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import evaluator_cases as EC  # noqa: E402
import forecast_ref as F  # noqa: E402
import loglik_unif_ref as U  # noqa: E402
import phasetype_amd as P  # noqa: E402
from phasetype_amd.synth import bd_exit, bd_exit_structure, simulate_ph  # noqa: E402

pytestmark = pytest.mark.gpu

ECS, UNIF = 2, 8
H1 = np.array([0.7])
H16 = np.concatenate([[0.0, 1e-9], np.geomspace(1e-3, 8.0, 14)])
ALL = F.KEYS + ("q", "M", "V", "nbad", "nunits", "p_unit")


def _gen(name):
    return U.ring(5) if name == "ring5" else bd_exit(int(name[2:]))


def _draws(S, s, nd):
    scales = np.linspace(0.8, 1.25, nd) if nd > 1 else np.array([1.0])
    return [S * c for c in scales], [s * c for c in scales]


def _fleet(units, seed=4):
    """``units`` censored observations with as many exact ones mixed in, in no
    order, ties among the ages (and between an exact and a censored one)"""
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
        return sw.forecast(Ss, ss, h, batch=batch, pointwise=True, grid_cap=grid_cap)
    finally:
        sw.close()


# censored units (1, 63, 64, 65: the wave's edges; 257, 1000: more than one
# block of 512, no multiple of it) x draws (1, 3, 65 with batch 64; 5 with
# batch 2: several batches, qsum in draw order across them) x H (1: the 4-slot
# kernel, 16: the 16-slot one) x generator
CASES = [(1, 1, 64, 1, "bd3"), (63, 3, 64, 16, "bd3"), (64, 65, 64, 1, "bd10"), (65, 5, 2, 16, "bd10"),
         (257, 3, 64, 16, "ring5"), (1000, 65, 64, 16, "bd10"), (1000, 5, 2, 1, "ring5"), (257, 1, 64, 16, "bd20"),
         (64, 3, 64, 16, "ring5"), (65, 65, 64, 1, "bd3"), (1000, 3, 64, 16, "bd3"), (1, 5, 2, 16, "ring5"),
         (63, 65, 64, 16, "bd10"), (257, 5, 2, 1, "bd3")]


@pytest.mark.parametrize("units,nd,batch,H,gen", CASES)
def test_bit_equal_to_the_restatement(gpu, units, nd, batch, H, gen):
    S, s = _gen(gen)
    Ss, ss = _draws(S, s, nd)
    y, cens = _fleet(units)
    h = H1 if H == 1 else H16
    got = _run(S.shape[0], y, cens, Ss, ss, h, batch=batch)
    want = F.forecast(Ss, ss, y, cens, h)
    assert F.same_bits(got, want, ALL) == []
    assert got["q"].shape == (nd, units, H) and np.all(np.isfinite(got["q"]))
    assert np.all(got["cnt"] == nd) and np.all(got["nunits"] == units)
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


TRUTH_ON_GPU = ("hypoexp-10", "stiff-12")


def _clean(r):
    """no draw flagged, no unit bad at any horizon, every value finite"""
    assert not r["flags"].any() and not r["bad_draw"].any() and not r["nbad"].any()
    for k in ("q", "M", "V", "p_unit", "qsum"):
        assert np.all(np.isfinite(r[k])), k


def _q_within_contract(S, s, y, cens, h, q):
    """q [units, H] of the draw (S, s) against the truth at every distinct age,
    within the header's contract from the context's table (as
    tests/test_forecast.py holds the restatement to it); the largest
    error / bound"""
    _, ages = F.units(y, cens)
    first = np.unique(ages, return_index=True)[1]
    truth = F.truth(S, s, ages[first], h)
    B = F.bound(S, s, ages[first], h, truth, ymax_c=float(np.max(ages)), hmax=float(h[-1]))
    worst = 0.0
    for i, u in enumerate(first):
        for j in range(len(h)):
            err = float(abs(truth[i][j] - float(q[u, j])))
            assert err <= B[i, j], (ages[u], h[j], err, B[i, j])
            if B[i, j] > 0:
                worst = max(worst, err / B[i, j])
    return worst


@pytest.mark.parametrize("case", EC.OFF_BD_GPU, ids=EC.case_id)
def test_off_bd_exit_bit_equal_to_the_restatement(gpu, sweepers, case):
    """The families of tests/evaluator_cases.py (single-successor rows, exact
    zeros in the forward vectors, a shift for R, rates over four decades):
    5 draws, 65 units among 130 observations with ties, the horizons within
    the table; batch 64 and 2.  On hypoexp10 and stiff12 the kernel's own q is
    held to the truth as well."""
    S, s, y, cens, h = EC.off_bd_case(case)
    Ss, ss = U.scaled(S, s)
    want = F.forecast(Ss, ss, y, cens, h)
    _clean(want)
    assert want["q"].shape == (5, 65, len(h)) and np.all(want["cnt"] == 5) and np.all(want["nunits"] == 65)
    sw = sweepers(S.shape[0])
    sw.set_obs(y, cens)
    for batch in (64, 2):
        got = sw.forecast(Ss, ss, h, batch=batch, pointwise=True)
        _clean(got)
        assert F.same_bits(got, want, ALL) == [], batch
        assert not got["q"][:, :, 0].any()  # h = 0
    if EC.case_id(case) in TRUTH_ON_GPU:
        worst = _q_within_contract(Ss[2], ss[2], y, cens, h, got["q"][2])
        print(f"{EC.case_id(case)}: the kernel's q, largest error / contract {worst:.4f}")


def test_table_sizes_mixed_in_one_call(gpu):
    """mu (ymax_c + h_max) = 1480 and 1465 for two of the draws (from 1457 on
    the sizing rule reaches the cap): K = 2047, one table an LDS pass; the
    others have K about 100 and share passes"""
    S, s = bd_exit(3)
    y, cens = _fleet(130)
    h = np.array([0.5, 8.0])
    ymax = float(np.max(y[cens != 0])) + 8.0
    mu0 = float(np.max(-np.diag(S)))
    big, small = 1480.0 / (mu0 * ymax), 10.0 / (mu0 * ymax)
    scales = [small, 1.2 * small, big, 0.9 * small, 0.99 * big, 1.1 * small, small]
    Ss, ss = [S * c for c in scales], [s * c for c in scales]
    Ks = [U.table(A, b, ymax)["K"] for A, b in zip(Ss, ss)]
    assert Ks[2] == 2047 and Ks[4] == 2047 and max(Ks[0], Ks[1], Ks[3]) < 150, Ks
    got = _run(3, y, cens, Ss, ss, h)
    want = F.forecast(Ss, ss, y, cens, h)
    assert F.same_bits(got, want, ALL) == []
    print("bad units per draw and horizon:", got["nbad"].tolist())
    assert not got["nbad"][0].any()


def test_bad_units_and_a_flagged_draw(gpu):
    S, s = bd_exit(3)
    Sn = S.copy()
    Sn[2, 1] = np.nan
    Ss, ss = [S, 0.9 * S, Sn, 1.1 * S], [s, 0.9 * s, s, 1.1 * s]
    y, cens = _fleet(65)
    h = np.array([1.0, 1e4])  # the second lies beyond every table
    got = _run(3, y, cens, Ss, ss, h)
    want = F.forecast(Ss, ss, y, cens, h)
    assert F.same_bits(got, want, ALL) == []
    assert got["bad_draw"].tolist() == [False, False, True, False] and got["flags"][2] == 4
    assert np.all(got["words"][2] == 0) and np.all(np.isnan(got["q"][2]))
    assert np.all(got["cnt"][:, 0] == 3) and np.all(got["cnt"][:, 1] == 0)
    good = [0, 1, 3]
    assert np.all(got["nbad"][good] == [0, 65]) and np.all(got["nunits"][good] == [65, 0])
    assert np.all(np.isfinite(got["q"][good][:, :, 0])) and np.all(np.isnan(got["q"][good][:, :, 1]))
    assert np.all(got["words"][good][:, 1, :2] == 0)


def test_callers_order_and_grid_independence(gpu):
    S, s = bd_exit(10)
    Ss, ss = _draws(S, s, 3)
    y, cens = _fleet(1000)
    base = _run(10, y, cens, Ss, ss, H16)
    for cap in (1, 3):
        assert F.same_bits(_run(10, y, cens, Ss, ss, H16, grid_cap=cap), base, ALL) == []
    perm = np.random.default_rng(1).permutation(len(y))
    got = _run(10, y[perm], cens[perm], Ss, ss, H16)
    assert np.array_equal(got["words"], base["words"])
    # unit r of the shuffled call is observation perm[unit_index[r]] of the first
    where = {int(i): r for r, i in enumerate(base["unit_index"])}
    rows = np.array([where[int(perm[i])] for i in got["unit_index"]])
    for k in ("qsum", "cnt", "p_unit"):
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(base[k][rows]).tobytes(), k
    assert got["q"].tobytes() == np.ascontiguousarray(base["q"][:, rows]).tobytes()
    # a DCS context keeps exact and censored observations in one sorted range
    assert F.same_bits(_run(10, y, cens, Ss, ss, H16, method=4), base, ALL) == []


def test_refusals(gpu):
    S, s = bd_exit(3)
    sw = P.Sweeper(3, ECS, 1, device=0)
    try:
        with pytest.raises(P.PhaseTypeError, match="no censored observation"):
            sw.forecast([S], [s], [1.0])
        sw.set_obs(np.array([1.0, 2.0]), np.zeros(2, np.int32))
        assert len(sw.forecast_units()) == 0
        with pytest.raises(P.PhaseTypeError, match="no censored observation"):
            sw.forecast([S], [s], [1.0])
        sw.set_obs(np.array([1.0, 2.0, 3.0]), np.array([0, 1, 1], np.int32))
        assert sw.forecast_units().tolist() == [1, 2]
        for h in ([], np.arange(17.0), [-1.0], [np.nan], [1.0, np.inf], [1.0, 1.0], [2.0, 1.0]):
            with pytest.raises(P.PhaseTypeError, match="horizon"):
                sw.forecast([S], [s], h)
        for batch in (0, 65):
            with pytest.raises(P.PhaseTypeError, match="batch"):
                sw.forecast([S], [s], [1.0], batch=batch)
        r = sw.forecast([S], [s], [1.0])
        assert r["nunits"].tolist() == [[2]] and "q" not in r and len(sw.last_forecast_ms) == 2
    finally:
        sw.close()


def test_waic_totals_and_chain_are_untouched(gpu):
    n, it = 3, 6
    T = np.zeros((4, 4), np.int32)
    T[0, 1], T[0, 3], T[1, 2], T[1, 3], T[2, 0], T[2, 3] = 1, 2, 3, 4, 5, 6
    theta = np.array([1.0, 0.1, 1.0, 0.1, 1.0, 0.1])
    S, s = P.theta_to_S(theta, T)
    y, cen = simulate_ph(S, s, 1000, seed=15, censor_frac=0.3)
    nu, zeta, Cm, zexp = 1 + 50 * theta, np.full(len(theta), 50.0), np.ones(T.shape), P.zexp_for(y)

    def run(with_f):
        P.set_seed(1)
        sw = P.Sweeper(n, UNIF, 1, device=0)
        sw.set_obs(y, cen)
        sw.waic_reset()
        if with_f:
            sw.forecast([S, 1.1 * S], [s, 1.1 * s], H16)
        a = sw.loglik_unif([S, 1.1 * S], [s, 1.1 * s], accumulate=True)
        if with_f:
            sw.forecast([S], [s], H1, batch=1, pointwise=True)
        c1 = sw.gibbs(it, UNIF, nu, zeta, T, Cm, zexp)
        if with_f:
            sw.forecast([0.9 * S] * 65, [0.9 * s] * 65, [0.5, 40.0])
        b = sw.loglik_unif([0.9 * S], [0.9 * s], accumulate=True)
        c2 = sw.gibbs(it, UNIF, nu, zeta, T, Cm, zexp, start=c1[-1])
        st = sw.waic_state()
        sw.close()
        return a, b, st, np.concatenate([c1, c2])

    wa, wb, wst, wc = run(True)
    a, b, st, c = run(False)
    for k in ("H", "F", "nbad", "nobs"):
        assert np.array_equal(wa[k], a[k]) and np.array_equal(wb[k], b[k]), k
    for k in ("ref", "S1", "S2", "m", "r"):
        assert np.ascontiguousarray(wst[k]).tobytes() == np.ascontiguousarray(st[k]).tobytes(), k
    assert np.array_equal(wst["cnt"], st["cnt"])
    assert wc.tobytes() == c.tobytes()


def test_fleet_forecast_at_size_within_contract(gpu):
    """n = 10, 2000 units, 64 draws through the public function.  The chain
    alternates between two parameter vectors, so p_unit is the mean of two
    values of q, each summed 32 times: the truth is the mean of the two
    truths, the bound the mean of the two contracts plus the rounding of the 63
    additions and the division (each at most 2^-53 of the final sum)."""
    n = 10
    T, theta = bd_exit_structure(n)
    S0, s0 = P.theta_to_S(theta, T)
    x, cen = simulate_ph(S0, s0, 2000, seed=33, censor_frac=0.0)
    cen = np.ones(2000, np.int32)
    res = np.stack([theta, 1.1 * theta] * 32)
    h = np.array([0.0, 0.1, 1.0, 3.0, 10.0])
    out = P.fleet_forecast(res, x, T, h, cen)
    assert out["p_unit"].shape == (2000, 5) and out["n_used"].tolist() == [64] * 5
    assert np.all(out["cnt"] == 64) and not out["nbad"].any()
    # the summary is the words'
    m = P.forecast_moments(out["M"], out["V"])
    for k in ("mean", "within", "between", "sd"):
        assert np.array_equal(out[k], m[k]), k
    assert np.all(np.diff(out["mean"]) > 0) and out["mean"][0] == 0 and np.all(out["sd"][1:] > 0)
    assert np.allclose(out["mean"], out["p_unit"].sum(0), rtol=1e-9, atol=1e-8)  # (2000 roundings to 2^-40)
    qs = out["count_quantiles"]([0.05, 0.5, 0.95])
    assert np.all(np.diff(qs[:, 1:], axis=0) > 0) and np.all(np.abs(qs[1, 1:] - out["mean"][1:]) < out["sd"][1:])
    # ranked by p_unit
    top = out["ranking"][3]
    assert np.all(np.diff(out["p_unit"][top, 3]) <= 0) and sorted(top) == list(range(2000))
    # 10 units x 5 horizons against the truth
    pick = np.argsort(x)[np.linspace(0, 1999, 10).astype(int)]
    ymax_c = float(np.max(x))
    draws = [P.theta_to_S(theta, T), P.theta_to_S(1.1 * theta, T)]
    truth = [np.array([[float(v) for v in row] for row in F.truth(S, s, x[pick], h)]) for S, s in draws]
    bound = [F.bound(S, s, x[pick], h, t, ymax_c=ymax_c) for (S, s), t in zip(draws, truth)]
    want = 0.5 * (truth[0] + truth[1])
    tol = 0.5 * (bound[0] + bound[1]) + 64 * 2.0 ** -53 * want
    err = np.abs(out["p_unit"][pick] - want)
    print(f"largest error / bound {np.max(err[:, 1:] / tol[:, 1:]):.3f}")
    assert np.all(err <= tol), (err, tol)
