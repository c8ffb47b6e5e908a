"""CPU: the specification of the posterior-predictive replicates
(include/pht_predict.h) through its C restatement (tests/predict_spec.c), the
host-only table builder of the library, and the numpy finalisation of ``ppc``.

Everything is deterministic under predict_ref.KEY.  Observed with that key at
R = 2 * 10^5 replicates (5-se bars against the analytic variances; the
Dvoretzky-Kiefer-Wolfowitz bound at alpha = 1e-9 is 0.007317):

    generator    z(mean)   z(jumps/path)   sup|ecdf - F|   the same, S scaled 1.1
    BD-exit(3)   -1.356    -1.134          0.001441        0.05126
    BD-exit(10)  -1.005    -0.261          0.002558        0.04540
    ring(5)      -0.441    +0.376          0.001984        0.04601
    n = 1        +0.597    (exactly 1)     0.001025        0.03514
"""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import phasetype_amd as P  # noqa: E402
import predict_ref as R  # noqa: E402

NREP = 200000
GENS = {"bd3": lambda: R.bd(3), "bd10": lambda: R.bd(10), "ring5": lambda: R.ring(5), "one": R.one_state}


def _edges(S):
    return np.linspace(0.05, 4.0, 64) * R.moments(S)[0]


@functools.lru_cache(maxsize=None)
def _run(name, scale=1.0):
    """the restatement's NREP replicates of a generator (computed once), on the
    64 edges of the unscaled generator"""
    S, s = GENS[name]()
    return R.predict([scale * S], [scale * s], NREP, edges=_edges(S))


@pytest.mark.parametrize("name", sorted(GENS))
def test_mean_against_the_analytic_moments(name):
    S, _ = GENS[name]()
    m1, m2 = R.moments(S)
    r = _run(name)
    assert r["ndone"][0] == NREP and r["nbad"][0] == 0 and r["nsurv"][0] == 0
    z = (r["mean"][0] - m1) / np.sqrt((m2 - m1 * m1) / NREP)
    print(f"{name}: mean {r['mean'][0]:.6f} m1 {m1:.6f} z {z:+.3f}; var {r['var'][0]:.6f} analytic {m2 - m1 * m1:.6f}")
    assert abs(z) <= 5.0
    # the unbiased variance agrees with the pointwise values' (a check of the exact sums, not a statistical one)
    assert abs(r["var"][0] - np.var(r["y"][0], ddof=1)) <= 1e-9 * r["var"][0]


@pytest.mark.parametrize("name", sorted(GENS))
def test_jumps_per_path_against_the_fundamental_matrix(name):
    S, _ = GENS[name]()
    jm, jv = R.jump_moments(S)
    r = _run(name)
    mean = r["njump"][0] / r["ndone"][0]
    if name == "one":
        assert jm == 1.0 and abs(jv) < 1e-12 and r["njump"][0] == r["ndone"][0]
        return
    z = (mean - jm) / np.sqrt(jv / NREP)
    print(f"{name}: jumps per path {mean:.5f} analytic {jm:.5f} z {z:+.3f}")
    assert abs(z) <= 5.0


@pytest.mark.parametrize("name", sorted(GENS))
def test_ecdf_within_dkw_and_rejects_a_scaled_generator(name):
    S, _ = GENS[name]()
    F = R.cdf(S, _edges(S))
    bound = R.dkw(NREP)
    D = float(np.max(np.abs(_run(name)["ecdf"][0] - F)))
    D_scaled = float(np.max(np.abs(_run(name, 1.1)["ecdf"][0] - F)))
    print(f"{name}: sup|ecdf - F| {D:.6f}, generator scaled 1.1: {D_scaled:.6f}, DKW bound {bound:.6f}")
    assert D <= bound
    assert D_scaled > bound  # power: the same check rejects a generator 10 % faster


def test_reductions_are_exact():
    S, s = R.ring(5)
    edges = _edges(S)[::4]
    nrep = 5000
    whole = R.predict([S, 0.9 * S], [s, 0.9 * s], nrep, edges=edges, draw0=3)
    # any split of the replicate range by rep0 adds up to the same words
    for cuts in ([0, 1, nrep], [0, 1234, 1235, 4000, nrep]):
        parts = [R.predict([S, 0.9 * S], [s, 0.9 * s], b - a, rep0=a, edges=edges, draw0=3)
                 for a, b in zip(cuts[:-1], cuts[1:])]
        comb = functools.reduce(P.predict_combine, parts)
        R.assert_same(whole, comb)
    for d in range(2):
        y = whole["y"][d]
        assert np.array_equal(whole["words"][d], R.words_from_y(y, whole["jumps"][d]))
        assert np.array_equal(whole["counts"][d], np.bincount(np.searchsorted(edges, y, "right"), minlength=len(edges) + 1))
        assert whole["ymin"][d] == y.min() and whole["ymax"][d] == y.max()
        assert np.array_equal(whole["ecdf"][d], np.cumsum(whole["counts"][d][:-1]) / nrep)
    # a replicate's value depends on its numbers alone: draw 1 of a call at draw0 = 3 is draw 0 at draw0 = 4
    alone = R.predict([0.9 * S], [0.9 * s], nrep, edges=edges, draw0=4)
    assert np.array_equal(R.bits(alone["y"][0]), R.bits(whole["y"][1]))


def test_horizon():
    S, s = R.bd(10)
    hz = R.moments(S)[0]
    free = R.predict([S], [s], 20000)
    cut = R.predict([S], [s], 20000, horizon=hz, edges=[0.5 * hz, hz])
    y, y0 = cut["y"][0], free["y"][0]
    assert cut["nsurv"][0] == np.sum(y == hz) and 0 < cut["nsurv"][0] < 20000
    assert np.all(y <= hz) and cut["ndone"][0] == 20000 and cut["nbad"][0] == 0
    early = y0 < hz
    assert np.array_equal(early, y < hz)
    assert np.array_equal(R.bits(y[early]), R.bits(y0[early]))
    assert np.array_equal(cut["jumps"][0][early], free["jumps"][0][early])
    assert np.all(cut["jumps"][0] <= free["jumps"][0])
    assert cut["counts"][0][2] == cut["nsurv"][0]  # recorded at the horizon: the bin of the edge that equals it
    assert np.array_equal(cut["words"][0], R.words_from_y(y, cut["jumps"][0], hz))


def test_jump_cap_makes_bad_replicates():
    S, s = R.ring(5, exit_div=1e3)
    assert R.jump_moments(S)[0] > 1000
    r = R.predict([S], [s], 2000, max_jumps=64, edges=[1.0, 10.0])
    assert r["nbad"][0] > 0 and r["ndone"][0] + r["nbad"][0] == 2000
    bad = np.isnan(r["y"][0])
    assert bad.sum() == r["nbad"][0]
    assert np.all(r["jumps"][0][bad] == 64) and np.all(r["jumps"][0] <= 64)
    assert r["counts"][0].sum() == r["ndone"][0]
    assert np.array_equal(r["words"][0], R.words_from_y(r["y"][0], r["jumps"][0]))
    # a recorded y >= 2^20 is bad as well: one state with rate 2^-30
    slow = R.predict([np.array([[-2.0 ** -30]])], [np.array([2.0 ** -30])], 200)
    assert slow["nbad"][0] > 150 and slow["ndone"][0] + slow["nbad"][0] == 200
    assert np.all(slow["y"][0][~np.isnan(slow["y"][0])] < 2.0 ** 20)


def _flag_cases():
    S, s = R.bd(3)
    nonfinite, zero_diag, negative = S.copy(), S.copy(), S.copy()
    nonfinite[1, 2] = np.nan
    zero_diag[1, 1] = 0.0
    negative[0, 1] = -2.0
    closed = np.array([[-2.0, 1.0, 1.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]])  # state 3 is reached and cannot leave
    return {"nonfinite": (nonfinite, s, P.LL_F_NONFINITE), "zero_diag": (zero_diag, s, P.LL_F_MU),
            "negative": (negative, s, P.PRED_F_RATE), "no_exit": (S, np.zeros(3), P.PRED_F_ABSORB),
            "closed_class": (closed, np.array([0.0, 1.0, 0.0]), P.PRED_F_ABSORB)}


@pytest.mark.parametrize("case", sorted(_flag_cases()))
def test_draw_flags(case):
    Sb, sb, bit = _flag_cases()[case]
    S, s = R.bd(3)
    assert R.table(Sb, sb)[0] == bit
    assert P.pred_table(Sb, sb)[0] == bit  # the library's host-only builder
    mid = R.predict([S, Sb, 1.1 * S], [s, sb, 1.1 * s], 300, edges=[0.5, 1.0])
    assert list(mid["flags"]) == [0, bit, 0] and list(mid["bad_draw"]) == [False, True, False]
    assert not mid["words"][1].any() and not mid["counts"][1].any() and np.all(np.isnan(mid["y"][1]))
    assert np.isnan(mid["mean"][1]) and np.isnan(mid["ymin"][1])
    for d, (Sd, sd) in ((0, (S, s)), (2, (1.1 * S, 1.1 * s))):  # the neighbours' words: as without the flagged draw
        alone = R.predict([Sd], [sd], 300, edges=[0.5, 1.0], draw0=d)
        assert np.array_equal(alone["words"][0], mid["words"][d]) and np.array_equal(alone["counts"][0], mid["counts"][d])


def test_an_unreachable_closed_class_is_not_flagged():
    S = np.array([[-1.0, 0.0], [0.0, -1.0]])
    assert R.table(S, np.array([1.0, 0.0]))[0] == 0


@pytest.mark.parametrize("name", sorted(GENS))
def test_pred_build_runs_without_a_device_and_equals_the_restatement(name):
    S, s = GENS[name]()
    n = S.shape[0]
    flag, tab = R.table(S, s)
    f2, scale, cum = P.pred_table(S, s)
    assert flag == 0 and f2 == 0 and P.load().pht_pred_words() == P.PRED_WORDS == 8
    assert np.array_equal(R.bits(tab[:n]), R.bits(scale)) and np.array_equal(R.bits(tab[n:]), R.bits(cum.reshape(-1)))
    assert np.array_equal(R.bits(scale), R.bits(1.0 / -np.diag(S)))
    for j in range(n):  # the running sums, by sequential additions in candidate order; +inf from the last positive one
        cand = [k for k in range(n) if k != j]
        pf = np.array([S[j, k] * scale[j] for k in cand] + [s[j] * scale[j]])
        last = int(np.nonzero(pf > 0)[0][-1])
        sums = np.array([functools.reduce(lambda a, b: a + b, pf[:q + 1], 0.0) for q in range(n)])
        assert np.array_equal(R.bits(cum[j, :last]), R.bits(sums[:last])) and np.all(np.isinf(cum[j, last:]))


def test_pred_build_refuses_bad_arguments():
    L = P.load()
    assert L.pht_pred_table_words(0) < 0 and L.pht_pred_table_words(33) < 0 and L.pht_pred_table_words(32) == 32 + 1024
    assert L.pht_pred_build(3, np.zeros(9), np.zeros(3), np.zeros(4), 4) < 0
    assert b"tab_words" in L.pht_last_error()


# ---------------------------------------------------------- ppc finalisation
def _hand_made():
    """three draws over edges (1, 2, 3): counts per bin, words to match"""
    edges = np.array([1.0, 2.0, 3.0])
    counts = np.array([[10, 20, 30, 40], [40, 30, 20, 10], [0, 0, 0, 0]])
    words = np.zeros((3, 8), np.int64)
    words[0, [0, 2, 4]] = [250, 725, 100]   # mean 2.5, var (725 - 625) / 99
    words[1, [0, 2, 4]] = [150, 325, 100]   # mean 1.5, var (325 - 225) / 99
    return P.predict_finalise(words, counts, [0.5, 0.25, np.inf], [3.5, 3.75, -np.inf], [0, 0, P.LL_F_MU], edges)


def test_predict_finalise_and_quantiles_from_counts():
    pred = _hand_made()
    assert list(pred["mean"][:2]) == [2.5, 1.5] and np.isnan(pred["mean"][2])
    assert np.allclose(pred["var"][:2], [100 / 99, 100 / 99]) and list(pred["bad_draw"]) == [False, False, True]
    assert np.array_equal(pred["ecdf"][0], [0.1, 0.3, 0.6]) and np.all(np.isnan(pred["ecdf"][2]))
    q = P.quantiles_from_counts(pred["counts"], pred["edges"], pred["ymin"], pred["ymax"], [0.1, 0.2, 0.5, 0.95, 1.0])
    # draw 0: rank 10 closes bin 0 at the edge 1; rank 20 is half way through bin 1 = [1, 2]; rank 50: 2/3 of [2, 3];
    # rank 95: 35/40 of [3, ymax = 3.5]; rank 100: ymax
    assert np.allclose(q[0], [1.0, 1.5, 2.0 + 2.0 / 3.0, 3.0 + 0.5 * 35 / 40, 3.5])
    assert np.allclose(q[1], [0.25 + 0.75 * 10 / 40, 0.25 + 0.75 * 20 / 40, 1.0 + 10 / 30, 3.0 + 0.75 * 0.5, 3.75])
    assert np.all(np.isnan(q[2]))


def test_ppc_p_value_arithmetic():
    pred = _hand_made()
    x = np.array([1.0, 2.0, 3.0, 2.0])  # mean 2, sd sqrt(2/3), min 1, max 3, median 2
    out = P.ppc_from_predict(pred, x, quantiles=(0.5,))
    assert out["n_draws_used"] == 2  # the flagged draw is left out
    assert out["p"]["mean"] == 0.5   # 2.5 >= 2, 1.5 < 2
    assert out["p"]["sd"] == 1.0     # sqrt(100 / 99) >= sqrt(2 / 3) twice
    assert out["p"]["min"] == 0.0 and out["p"]["max"] == 1.0
    assert out["p"]["q0.5"] == 0.5   # medians 2.667 and 1.333 against 2
    assert np.array_equal(out["ecdf_x"], [0.0, 0.25, 0.75])  # the share of the data below each edge
    assert out["band"].shape == (3, 3) and np.allclose(out["band"][1], [0.25, 0.5, 0.75])
    assert np.all(out["band"][0] <= out["band"][1]) and np.all(out["band"][1] <= out["band"][2])
    comb = P.predict_combine(pred, pred)
    assert np.array_equal(comb["words"], 2 * pred["words"]) and np.array_equal(comb["counts"], 2 * pred["counts"])
    assert list(comb["ymin"][:2]) == [0.5, 0.25] and list(comb["mean"][:2]) == [2.5, 1.5]


def test_ppc_refuses_censored_data_without_a_horizon():
    x = np.array([1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="horizon"):
        P.ppc(np.ones((2, 7)), x, None, censored=[0, 0, 1])
    with pytest.raises(ValueError, match="equal"):
        P.ppc(np.ones((2, 7)), x, None, censored=[0, 1, 0], horizon=3.0)  # a censored observation away from the horizon
