"""CPU: the fleet-forecast specification (include/pht_forecast.h) through the
tests' restatement (tests/forecast_spec.c), the host-only library function and
the Python layer; no GPU.

* pht_fc_q against mpmath within the header's recorded r, exactly 0 at
  dl >= 0, monotone across the threshold.
* The restatement against the truth (mpmath) within the header's contract and
  nothing else, off BD-exit too.
* h = 0, monotone in h, q -> 1; a horizon beyond the table makes units bad,
  never a finite wrong value.
* The words add over shards bit for bit; forecast_combine agrees.
* fleet_forecast's moments, count_quantiles against the exact mixture of
  Poisson-binomial laws, the refusals of pht_forecast_host.
"""
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
THRESH = -0.25


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def scattered(S, s, draws, sigma=0.15, seed=5):
    """``draws`` generators: every rate of (S, s) times exp(sigma N(0, 1))"""
    rng = np.random.default_rng(seed)
    Ss, ss = [], []
    for _ in range(draws):
        A = S * np.exp(sigma * rng.standard_normal(S.shape))
        b = s * np.exp(sigma * rng.standard_normal(s.shape))
        np.fill_diagonal(A, 0.0)
        np.fill_diagonal(A, -(A.sum(1) + b))
        Ss.append(A)
        ss.append(b)
    return Ss, ss


# ------------------------------------------------------------------ pht_fc_q
def fc_q_grid(points=20000):
    """-1e-300 .. -700 log-uniformly, -1e-3 .. -10 and -0.2 .. -0.3 densely, and
    the 50 doubles on either side of the threshold (the header's measurement
    took this grid with points = 200000)"""
    a = -np.logspace(-300, np.log10(700.0), points - points // 5 + 1)
    b = -np.linspace(0.2, 0.3, points // 10)
    c = -np.logspace(-3, 1, points // 10)
    near, lo, hi = [THRESH], THRESH, THRESH
    for _ in range(50):
        lo, hi = np.nextafter(lo, -1.0), np.nextafter(hi, 0.0)
        near += [lo, hi]
    return np.concatenate([a, b, c, near])


def test_header_constants():
    L = F.spec()
    assert L.fspec_maxh() == 16 == P.FORECAST_MAX_H
    assert L.fspec_maxunits() == 1 << 22 == P.FORECAST_MAX_UNITS
    assert L.fspec_thresh() == THRESH and L.fspec_scale() == 2.0 ** 40
    assert L.fspec_r() == 3 * 2.0 ** -53


def test_fc_q_within_recorded_r():
    import mpmath as mp

    dl = fc_q_grid()
    q = F.fc_q(dl)
    r = F.spec().fspec_r()
    worst = {"polynomial": 0.0, "1 - exp": 0.0}
    with mp.workdps(60):
        for x, v in zip(dl, q):
            t = -mp.expm1(mp.mpf(float(x)))
            e = float(abs(mp.mpf(float(v)) - t) / t)
            k = "polynomial" if x > THRESH else "1 - exp"
            worst[k] = max(worst[k], e)
    print({k: f"{v * 2.0 ** 53:.2f} x 2^-53" for k, v in worst.items()}, f"r = {r * 2.0 ** 53:g} x 2^-53")
    assert max(worst.values()) <= r, worst
    assert np.all((q > 0) & (q <= 1))
    assert F.fc_q([-800.0, -np.inf]).tolist() == [1.0, 1.0]


def test_fc_q_zero_for_non_negative():
    q = F.fc_q([0.0, -0.0, 5e-324, 1e-300, 1e-17, 0.3, 5.0, 800.0, np.inf])
    assert _bits(q) == _bits(np.zeros(9))


def test_fc_q_monotone_across_threshold():
    """non-increasing in dl wherever the true values differ by more than 2 r q:
    steps of 2^-44 in dl change q by at least e^-0.26 2^-44 = 4.4e-14, the
    function's error is at most r q < 3.4e-16 0.23 there"""
    k = np.arange(-4096, 4097)
    dl = THRESH + k * 2.0 ** -44
    assert dl[4095] < THRESH < dl[4097] and dl[4096] == THRESH
    q = F.fc_q(dl)
    assert np.all(np.diff(q) < 0)
    # and on a coarse grid over the whole range
    dl = -np.logspace(-12, 2.8, 3000)[::-1]
    assert np.all(np.diff(F.fc_q(dl)) <= 0)


# ------------------------------------------------- restatement against truth
def _mu(S):
    return float(np.max(-np.diag(S)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_within_contract(name):
    S, s = CASES[name]()
    y, cens = AGES, np.ones(len(AGES), np.int32)
    r = F.forecast([S], [s], y, cens, HORIZONS)
    assert not r["bad_draw"][0]
    q = r["q"][0]
    # a cell is bad only beyond the documented limit mu (c + h) <= 1400
    reach = _mu(S) * (AGES[:, None] + HORIZONS[None, :])
    bad = np.isnan(q)
    assert not np.any(bad & (reach <= EC.MU_Y_MAX)), (name, np.argwhere(bad & (reach <= EC.MU_Y_MAX)))
    if not name.startswith("stiff"):  # (their largest rate is 250: only c + h up to 5.6 lies inside the table)
        assert not bad.any()
    assert (~bad[:, HORIZONS > 0]).sum() >= 12, (name, bad)
    worst, cells = 0.0, 0
    for i, c in enumerate(AGES):
        good = np.flatnonzero(~bad[i])
        if not len(good):
            continue
        truth = F.truth(S, s, [c], HORIZONS[good])
        # the contract's bound, from the table of the whole context
        B = F.bound(S, s, [c], HORIZONS[good], truth, ymax_c=float(np.max(AGES)), hmax=float(HORIZONS[-1]))
        for a, j in enumerate(good):
            err = float(abs(truth[0][a] - float(q[i, j])))
            assert err <= B[0, a], (name, c, HORIZONS[j], err, B[0, a])
            cells += 1
            if B[0, a] > 0:
                worst = max(worst, err / B[0, a])
    print(f"{name}: worst error / contract = {worst:.3f} over {cells} cells")
    assert r["nunits"][0].tolist() == (~bad).sum(0).tolist() and r["nbad"][0].tolist() == bad.sum(0).tolist()


def test_host_function_equals_restatement():
    S, s = bd_exit(3)
    Ss, ss = scattered(S, s, 3)
    ages = np.array([0.3, 2.0, 2.0, 7.5, 1e-6])
    want = F.forecast(Ss, ss, ages, np.ones(5, np.int32), HORIZONS)
    st = None
    for d in range(3):
        st = P.forecast_host(Ss[d], ss[d], ages, HORIZONS, state=st)
        assert _bits(st["words"][0]) == _bits(want["words"][d]) and _bits(st["q"][0]) == _bits(want["q"][d])
    assert _bits(st["qsum"]) == _bits(want["qsum"]) and _bits(st["cnt"]) == _bits(want["cnt"])
    assert _bits(st["p_unit"]) == _bits(want["p_unit"])


# -------------------------------------------------------------- worded cases
def test_zero_horizon_is_exactly_zero():
    S, s = bd_exit(10)
    r = F.forecast([S], [s], AGES, np.ones(len(AGES), np.int32), [0.0])
    assert _bits(r["q"]) == _bits(np.zeros((1, len(AGES), 1)))
    assert r["words"][0, 0].tolist() == [0, 0, 0, len(AGES)]
    assert _bits(r["M"]) == _bits(np.zeros((1, 1))) and _bits(r["V"]) == _bits(np.zeros((1, 1)))


def test_monotone_in_horizon_and_tends_to_one():
    S, s = bd_exit(3)
    h = np.array([0.0, 1e-9, 1e-3, 0.1, 1.0, 10.0, 50.0, 150.0])
    r = F.forecast([S], [s], AGES, np.ones(len(AGES), np.int32), h)
    q = r["q"][0]
    assert np.all(np.isfinite(q)) and np.all(np.diff(q, axis=1) >= 0)
    # Fbar(c + 150) / Fbar(c) decays like the slowest rate: far below 1e-9 here
    assert np.all(q[:, -1] > 1 - 1e-9) and np.all(q <= 1.0)
    assert abs(r["M"][0, -1] - len(AGES)) < 1e-8 and r["V"][0, -1] < 1e-8


def test_horizon_beyond_table_makes_units_bad():
    """mu (c + h) past the table's cap: the units are bad at that horizon only,
    counted, never summed, never a finite value"""
    S, s = bd_exit(3)
    Ss, ss = scattered(S, s, 2)
    ages = np.array([0.5, 3.0, 3.0])
    h = np.array([1.0, 1e4])
    assert _mu(S) * 1e4 > 2047
    r = F.forecast(Ss, ss, ages, np.ones(3, np.int32), h)
    assert not r["bad_draw"].any()
    assert np.all(np.isfinite(r["q"][:, :, 0])) and np.all(np.isnan(r["q"][:, :, 1]))
    assert r["nbad"].tolist() == [[0, 3], [0, 3]] and r["nunits"].tolist() == [[3, 0], [3, 0]]
    assert np.all(r["words"][:, 1, :2] == 0) and np.all(r["words"][:, 0, 0] > 0)
    assert r["cnt"].tolist() == [[2, 0]] * 3 and np.all(r["qsum"][:, 1] == 0)
    assert np.all(np.isnan(r["p_unit"][:, 1])) and np.all(np.isfinite(r["p_unit"][:, 0]))


def test_flagged_draw_is_skipped():
    S, s = bd_exit(3)
    Sn = S.copy()
    Sn[1, 2] = np.nan
    ages = np.array([0.5, 3.0])
    r = F.forecast([S, Sn, S], [s, s, s], ages, np.ones(2, np.int32), [0.5, 2.0])
    assert r["bad_draw"].tolist() == [False, True, False] and r["flags"][1] == 4
    assert np.all(r["words"][1] == 0) and np.all(np.isnan(r["q"][1]))
    assert np.all(r["cnt"] == 2)
    assert _bits(r["words"][0]) == _bits(r["words"][2])


# ---------------------------------------------------------------- the words
def _fleet(N, seed=2):
    rng = np.random.default_rng(seed)
    y = np.round(rng.exponential(3.0, N), 3) + 1e-3  # ties among the ages
    cens = (rng.random(N) < 0.5).astype(np.int32)
    cens[:2] = (1, 0)
    return y, cens


def test_words_add_over_shards_and_combine_agrees():
    S, s = bd_exit(3)
    Ss, ss = scattered(S, s, 4)
    y, cens = _fleet(80)
    whole = F.forecast(Ss, ss, y, cens, HORIZONS)
    a = F.forecast(Ss, ss, y[:50], cens[:50], HORIZONS)  # each shard's table from its own largest censored age
    b = F.forecast(Ss, ss, y[50:], cens[50:], HORIZONS)
    assert _bits(a["words"] + b["words"]) == _bits(whole["words"])
    c = P.forecast_combine(a, b)
    for k in ("words", "M", "V", "nbad", "nunits", "qsum", "cnt", "p_unit", "q", "flags"):
        assert _bits(c[k]) == _bits(whole[k]), k
    assert np.array_equal(c["unit_index"], np.concatenate([a["unit_index"], b["unit_index"]]))
    assert np.array_equal(np.concatenate([a["unit_index"], b["unit_index"] + 50]), whole["unit_index"])
    # M and V are the sums they are said to be
    q = whole["q"]
    assert np.array_equal(whole["words"][:, :, 0], np.rint(q * 2.0 ** 40).astype(np.int64).sum(1))
    assert np.array_equal(whole["words"][:, :, 1], np.rint(q * (1 - q) * 2.0 ** 40).astype(np.int64).sum(1))
    with pytest.raises(ValueError):
        P.forecast_combine(a, F.forecast(Ss[:3], ss[:3], y[50:], cens[50:], HORIZONS))


# --------------------------------------------------------------- the summary
def test_moments_from_hand_made_words():
    M = np.array([[1.0, 10.0], [3.0, 14.0], [2.0, 12.0], [6.0, 99.0]])
    V = np.array([[0.5, 4.0], [1.5, 6.0], [1.0, 2.0], [3.0, 99.0]])
    use = np.array([[1, 1], [1, 1], [1, 1], [1, 0]], bool)
    m = P.forecast_moments(M, V, use)
    assert m["n_used"].tolist() == [4, 3]
    assert np.allclose(m["mean"], [3.0, 12.0], rtol=0, atol=1e-15)
    assert np.allclose(m["within"], [1.5, 4.0], rtol=0, atol=1e-15)
    assert np.allclose(m["between"], [3.5, 8.0 / 3.0], rtol=1e-15, atol=0)
    assert np.allclose(m["sd"], np.sqrt([5.0, 4.0 + 8.0 / 3.0]), rtol=1e-15, atol=0)
    # one draw: no spread between draws
    one = P.forecast_moments(M[:1], V[:1])
    assert one["between"].tolist() == [0.0, 0.0] and np.allclose(one["sd"], np.sqrt(V[0]))
    # a single normal: the mixture's quantiles are its own
    qs = P.forecast_count_quantiles([[10.0]], [[4.0]], [0.5, 0.8413447460685429])
    assert np.allclose(qs[:, 0], [10.0, 12.0], rtol=0, atol=1e-9)


# recorded in DESIGN.md 5i: the largest |count_quantiles - exact| in counts over
# p in COUNT_P and the three horizons of this fleet (200 units, 50 draws)
COUNT_P = (.05, .25, .5, .75, .95)
COUNT_DIFF_MEASURED = 0.51


def test_count_quantiles_against_exact_mixture():
    S, s = bd_exit(3)
    Ss, ss = scattered(S, s, 50, sigma=0.3)
    rng = np.random.default_rng(9)
    ages = rng.exponential(2.0, 200) + 0.01
    h = np.array([0.1, 1.0, 5.0])
    r = F.forecast(Ss, ss, ages, np.ones(200, np.int32), h)
    assert np.all(np.isfinite(r["q"]))
    got = P.forecast_count_quantiles(r["M"], r["V"], COUNT_P)
    worst = 0.0
    for j in range(len(h)):
        pmf = np.mean([F.poisson_binomial(r["q"][d, :, j]) for d in range(50)], axis=0)
        cdf = np.cumsum(pmf)
        # the moments of the exact law are the words'
        k = np.arange(201)
        mom = P.forecast_moments(r["M"][:, j:j + 1], r["V"][:, j:j + 1])
        assert abs(float(pmf @ k) - mom["mean"][0]) < 1e-6
        assert abs(float(pmf @ k ** 2) - float(pmf @ k) ** 2 - mom["sd"][0] ** 2) < 1e-6
        for i, p in enumerate(COUNT_P):
            exact = int(np.searchsorted(cdf, p - 1e-12))
            worst = max(worst, abs(got[i, j] - exact))
            print(f"h = {h[j]:g} p = {p:g}: exact {exact} normal mixture {got[i, j]:.3f}")
    print(f"largest difference {worst:.3f} counts (recorded: {COUNT_DIFF_MEASURED})")
    assert worst <= COUNT_DIFF_MEASURED + 1.0


# ---------------------------------------------------------------- refusals
def test_host_refusals():
    S, s = bd_exit(3)
    ok = np.array([1.0, 2.0])
    P.forecast_host(S, s, ok, [0.5])
    for ages, h, what in [
        (np.zeros(0), [0.5], "no censored unit"),
        (ok, [], "horizons"),
        (ok, np.arange(17.0), "horizons"),
        (ok, [-1.0], "horizon"),
        (ok, [np.nan], "horizon"),
        (ok, [1.0, np.inf], "horizon"),
        (ok, [1.0, 1.0], "horizon"),
        (ok, [2.0, 1.0], "horizon"),
    ]:
        with pytest.raises(P.PhaseTypeError, match=what):
            P.forecast_host(S, s, ages, h)
    with pytest.raises(P.PhaseTypeError, match="at most"):
        P.forecast_host(S, s, np.ones((1 << 22) + 1), [0.5])
    with pytest.raises(P.PhaseTypeError, match="ymax_c"):
        P.forecast_host(S, s, ok, [0.5], ymax_c=1.5)
    assert P.forecast_host(S, s, ok, np.arange(16.0))["q"].shape == (1, 2, 16)
