"""GPU: the uniformisation log-likelihood kernels
(phasetype_amd/csrc/pht_loglik_unif.hip) against the CPU restatement of
include/pht_loglik_unif.h (tests/loglik_unif_spec.c) bit for bit: pointwise
values, the int64 totals words, the WAIC state; batching, sharding, partial
waves and the staging of tables of mixed length; evaluator="auto" in draw
order; a UNIF sampler's chain untouched; the Python API end to end."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import evaluator_cases as EC  # noqa: E402
import loglik_ref as R  # noqa: E402
import loglik_unif_ref as U  # noqa: E402
import phasetype_amd as P  # noqa: E402
from phasetype_amd.synth import bd_exit, simulate_ph  # noqa: E402

pytestmark = pytest.mark.gpu

ECS, DCS, UNIF = 2, 4, 8
WAIC_KEYS = ("ref", "S1", "S2", "m", "r", "cnt")
WORDS = ("H", "F", "nbad", "nobs")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _words(r):
    return np.stack([r[k] for k in WORDS], axis=1)


def _gen(n):
    return U.CYCLIC if n == 3 else U.ring(n)


def _case(n, N, seed=11, edges=True):
    """(S_list, s_list, y, cens, restatement's l[draw, obs]): CYCLIC (n = 3) or
    ring(n), scaled by 0.8 .. 1.25; N observations, 30 % censored, plus the
    edge y's."""
    S, s = _gen(n)
    y, cens = simulate_ph(S, s, N, seed=seed, censor_frac=0.3)
    if edges:
        y, cens = U.with_edges(y, cens)
    Ss, ss = U.scaled(S, s)
    return Ss, ss, y, cens, U.pointwise(Ss, ss, y, cens)


def _sweeper(n, y, cens, method=ECS):
    sw = P.Sweeper(n, method, 1, device=0)
    sw.set_obs(y, cens)
    return sw


def _same_state(got, want, tag=None):
    for k in WAIC_KEYS:
        assert np.array_equal(got[k], want[k]) and np.array_equal(_bits(got[k].astype(np.float64)),
                                                                  _bits(want[k].astype(np.float64))), (tag, k)


@pytest.fixture(scope="module")
def case5(gpu):
    return _case(5, 2000)


@pytest.mark.parametrize("n", [3, 7, 10, 20, 32])
def test_pointwise_bit_exact(gpu, n):
    Ss, ss, y, cens, want = _case(n, 2000)
    assert np.all(np.isfinite(want))
    sw = _sweeper(n, y, cens)
    assert sw.loglik_unif_K(np.max(-np.diag(Ss[0]))) == U.table(Ss[0], ss[0], y.max())["K"]
    got = sw.loglik_unif(Ss, ss, pointwise=True)
    sw.close()
    assert np.array_equal(_bits(got["pointwise"]), _bits(want))
    assert np.array_equal(_words(got), R.totals(want))
    assert not got["bad_draw"].any() and not got["flags"].any() and np.all(np.isfinite(got["total"]))


@pytest.mark.parametrize("n", [3, 10])
@pytest.mark.parametrize("family", EC.FAMILIES)
def test_pointwise_bit_exact_off_bd_exit(gpu, family, n):
    """Real spectra off BD-exit (tests/evaluator_cases.py: stiff, defective
    and nearly defective among them), scaled by 0.8 .. 1.25, over 65
    observations from y = 1e-9 to 60, exact and censored interleaved: batch 1
    and 64, totals-only and pointwise, no observation bad."""
    S, s = EC.generator(family, n, **({"eps": 1e-3} if family == "gapped" else {}))
    Ss, ss = U.scaled(S, s)
    y, cens = EC.tiled(*EC.observations(S, scale=max(U.SCALES)), 65)
    want = U.pointwise(Ss, ss, y, cens)
    assert np.all(np.isfinite(want))
    sw = _sweeper(n, y, cens)
    for batch in (1, 64):
        got = sw.loglik_unif(Ss, ss, batch=batch)
        assert np.array_equal(_words(got), R.totals(want)), batch
        got = sw.loglik_unif(Ss, ss, batch=batch, pointwise=True)
        assert np.array_equal(_bits(got["pointwise"]), _bits(want)), batch
        assert np.array_equal(_words(got), R.totals(want)), batch
        assert not got["flags"].any() and np.all(np.isfinite(got["total"]))
    sw.close()


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_shapes_and_batches(gpu, N):
    n = 5
    Ss, ss, y, cens, want = _case(n, N, seed=12, edges=False)
    tot = R.totals(want)
    st = R.waic_state(want)
    sw = _sweeper(n, y, cens)
    for batch in (1, 2, 5, 64):
        sw.waic_reset()
        got = sw.loglik_unif(Ss, ss, batch=batch, accumulate=True)
        assert np.array_equal(_words(got), tot), batch
        _same_state(sw.waic_state(), st, batch)
        pw = sw.loglik_unif(Ss, ss, batch=batch, pointwise=True)["pointwise"]
        assert np.array_equal(_bits(pw), _bits(want)), batch
    sw.close()


def test_tables_of_mixed_length_in_a_batch(gpu):
    """A draw whose table is at the cap (it fills a staging pass alone) among
    draws with short tables; then an observation beyond the cap, bad for that
    draw only."""
    n = 5
    S, s = U.ring(n)
    y, cens = simulate_ph(S, s, 300, seed=13, censor_frac=0.3)
    big = 1500.0 / (4.0 * y.max())  # mu = 4: mu y_max = 1500, K at the cap
    scales = (1.0, 0.9, big, 1.1, big * 0.999, 0.8, 1.25)
    Ss, ss = U.scaled(S, s, scales)
    Ks = [U.table(a, b, y.max())["K"] for a, b in zip(Ss, ss)]
    assert Ks[2] == Ks[4] == 2047 and max(Ks[:2] + Ks[3:4] + Ks[5:]) < 300
    want = U.pointwise(Ss, ss, y, cens)
    assert np.all(np.isfinite(want))
    sw = _sweeper(n, y, cens)
    for batch in (64, 3):
        sw.waic_reset()
        got = sw.loglik_unif(Ss, ss, batch=batch, pointwise=True, accumulate=True)
        assert np.array_equal(_bits(got["pointwise"]), _bits(want)), batch
        assert np.array_equal(_words(got), R.totals(want)), batch
        _same_state(sw.waic_state(), R.waic_state(want), batch)
    sw.close()
    y2, cens2 = np.append(y, 1.5 * y.max()), np.append(cens, 0).astype(np.int32)
    want2 = U.pointwise(Ss, ss, y2, cens2)
    assert np.isnan(want2[[2, 4], -1]).all() and np.isfinite(np.delete(want2, [2, 4], axis=0)).all()
    sw = _sweeper(n, y2, cens2)
    got = sw.loglik_unif(Ss, ss, pointwise=True)
    sw.close()
    assert np.array_equal(_bits(got["pointwise"]), _bits(want2))
    assert got["nbad"].tolist() == [0, 0, 1, 0, 1, 0, 0] and np.all(got["nobs"] + got["nbad"] == len(y2))
    assert np.isneginf(got["total"][[2, 4]]).all() and np.isfinite(np.delete(got["total"], [2, 4])).all()
    assert np.array_equal(_words(got), R.totals(want2))


def test_shards_add_to_the_whole(gpu, case5):
    Ss, ss, y, cens, want = case5
    words = []
    for lo, hi in ((0, len(y)), (0, 777), (777, len(y))):
        sw = _sweeper(5, y[lo:hi], cens[lo:hi])
        words.append(_words(sw.loglik_unif(Ss, ss)))
        sw.close()
    assert np.array_equal(words[1] + words[2], words[0])
    assert np.array_equal(words[0], R.totals(want))


def test_dcs_context_returns_the_callers_order(gpu, case5):
    Ss, ss, y, cens, want = case5
    sw = _sweeper(5, y, cens, DCS)
    got = sw.loglik_unif(Ss, ss, pointwise=True)["pointwise"]
    sw.close()
    assert np.array_equal(_bits(got), _bits(want))


def test_flagged_draw_in_a_batch(gpu, case5):
    Ss, ss, y, cens, want = case5
    Sn = Ss[1].copy()
    Sn[2, 1] = np.nan
    sw = _sweeper(5, y, cens)
    got = sw.loglik_unif([Ss[0], Sn, Ss[2]], [ss[0], ss[1], ss[2]], pointwise=True, accumulate=True)
    st = sw.waic_state()
    sw.close()
    assert got["flags"].tolist() == [0, 4, 0] and got["bad_draw"].tolist() == [False, True, False]
    assert np.all(np.isnan(got["pointwise"][1])) and np.isnan(got["total"][1])
    assert _words(got)[1].tolist() == [0, 0, 0, 0]
    assert np.array_equal(_bits(got["pointwise"][[0, 2]]), _bits(want[[0, 2]]))
    _same_state(st, R.waic_state(want[[0, 2]]))


def test_auto_keeps_the_draw_order(gpu):
    n = 3
    S, s = bd_exit(n)
    real = [(S * c, s * c) for c in (0.9, 1.0, 1.1)]
    cyc = [(U.CYCLIC[0] * c, U.CYCLIC[1] * c) for c in (1.0, 0.9, 1.2)]
    seq = [real[0], real[1], cyc[0], real[2], cyc[1], cyc[2]]
    is_cyc = np.array([False, False, True, False, True, True])
    Ss, ss = [d[0] for d in seq], [d[1] for d in seq]
    y, cens = simulate_ph(S, s, 500, seed=14, censor_frac=0.3)
    sw = _sweeper(n, y, cens)
    blocks = np.stack([P.loglik_block(a, b) for a, b in real])
    spectral = sw.loglik_blocks(blocks, pointwise=True)
    unif = sw.loglik_unif([d[0] for d in cyc], [d[1] for d in cyc], pointwise=True)
    sw.waic_reset()
    got = sw.loglik(Ss, ss, pointwise=True, accumulate=True, evaluator="auto")
    st = sw.waic_state()
    dflt = sw.loglik(Ss, ss)
    sw.close()
    assert got["evaluator"].tolist() == ["unif" if c else "spectral" for c in is_cyc]
    assert not got["bad_draw"].any() and np.all(np.isfinite(got["total"]))
    for k in WORDS:
        assert np.array_equal(got[k][~is_cyc], spectral[k]), k
        assert np.array_equal(got[k][is_cyc], unif[k]), k
    assert np.array_equal(_bits(got["pointwise"][~is_cyc]), _bits(spectral["pointwise"]))
    assert np.array_equal(_bits(got["pointwise"][is_cyc]), _bits(unif["pointwise"]))
    # the restatements' mixed pointwise matrix, sequentially
    mixed = np.zeros((6, len(y)))
    mixed[~is_cyc] = R.pointwise(blocks, y, cens)
    mixed[is_cyc] = U.pointwise([d[0] for d in cyc], [d[1] for d in cyc], y, cens)
    assert np.array_equal(_bits(got["pointwise"]), _bits(mixed))
    assert np.all(st["cnt"] == 6)
    _same_state(st, R.waic_state(mixed))
    # the default is unchanged: the cyclic draws are NaN
    assert dflt["bad_draw"].tolist() == is_cyc.tolist() and np.all(np.isnan(dflt["total"][is_cyc]))
    assert dflt["evaluator"].tolist() == ["spectral"] * 6


def _cyclic_structure():
    """T of the 3-cycle 1 -> 2 -> 3 -> 1 with an exit from every state, and a
    chain's rows around CYCLIC's rates."""
    T = np.zeros((4, 4), np.int32)
    T[0, 1], T[0, 3], T[1, 2], T[1, 3], T[2, 0], T[2, 3] = 1, 2, 3, 4, 5, 6
    theta = np.array([1.0, 0.1, 1.0, 0.1, 1.0, 0.1])
    return T, theta


def test_unif_sampler_chain_is_untouched(gpu):
    n, it = 3, 6
    T, theta = _cyclic_structure()
    S, s = P.theta_to_S(theta, T)
    y, cen = simulate_ph(S, s, 1000, seed=15, censor_frac=0.3)
    nu, zeta, Cm, zexp = 1 + 50 * theta, np.full(len(theta), 50.0), np.ones(T.shape), P.zexp_for(y)

    def chain(with_loglik):
        P.set_seed(1)
        sw = _sweeper(n, y, cen, UNIF)
        if with_loglik:
            sw.loglik_unif([S, 1.1 * S], [s, 1.1 * s], accumulate=True)
        a = sw.gibbs(it, UNIF, nu, zeta, T, Cm, zexp)
        if with_loglik:
            sw.loglik_unif([S], [s], pointwise=True)
        b = sw.gibbs(it, UNIF, nu, zeta, T, Cm, zexp, start=a[-1])
        sw.close()
        return np.concatenate([a, b])

    assert np.array_equal(_bits(chain(True)), _bits(chain(False)))


def test_end_to_end_cyclic_structure(gpu):
    n = 3
    T, theta = _cyclic_structure()
    S, s = P.theta_to_S(theta, T)
    y, cen = simulate_ph(S, s, 1000, seed=16, censor_frac=0.3)
    rows = np.stack([theta * c for c in (0.8, 0.9, 1.0, 1.1, 1.25)])
    ll = P.log_lik(rows, y, T, censored=cen, evaluator="auto")
    assert ll.shape == (5,) and np.all(np.isfinite(ll))
    assert np.all(np.isnan(P.log_lik(rows, y, T, censored=cen, evaluator="spectral")))
    assert np.all(np.isnan(P.log_lik(rows, y, T, censored=cen)))
    sw = _sweeper(n, y, cen)
    for k in range(5):
        Sk, sk = P.theta_to_S(rows[k], T)
        assert sw.loglik_unif([Sk], [sk])["total"][0] == ll[k], k
    sw.close()
    w = P.waic(rows, y, T, censored=cen, burn=1, evaluator="auto")
    assert w["n_draws_used"] == 4 and np.isfinite(w["waic"]) and w["p_waic"] > 0
    assert P.waic(rows, y, T, censored=cen, burn=1)["n_draws_used"] == 0


def test_ph_curves_unif(gpu):
    T, theta = _cyclic_structure()
    rows = np.stack([theta * c for c in (0.9, 1.0, 1.1)])
    grid = np.concatenate([[1e-9], np.linspace(0.05, 8.0, 32)])
    out = P.ph_curves(rows, T, grid, evaluator="unif")
    assert out["logdens"].shape == out["logsurv"].shape == out["hazard"].shape == (3, 33)
    assert np.all(np.isfinite(out["logdens"])) and np.all(np.isfinite(out["logsurv"]))
    assert np.array_equal(out["hazard"], np.exp(out["logdens"] - out["logsurv"]))
    assert np.all(np.diff(out["logsurv"], axis=1) <= 0)
    for d, c in enumerate((0.9, 1.0, 1.1)):
        assert abs(out["logdens"][d, 0] - np.log(0.1 * c)) <= 1e-8
