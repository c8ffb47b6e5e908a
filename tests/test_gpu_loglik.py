"""GPU: the log-likelihood kernel (phasetype_amd/csrc/pht_loglik.hip) against
the CPU restatement of include/pht_loglik.h (tests/loglik_spec.c) bit for
bit: pointwise values, the int64 totals words, the WAIC state; batching,
sharding and partial waves; flagged draws; the Python API end to end."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import loglik_ref as R  # noqa: E402
import phasetype_amd as P  # noqa: E402
from phasetype_amd.synth import bd_exit, bd_exit_structure, simulate_ph  # noqa: E402

pytestmark = pytest.mark.gpu

ECS = 2
WAIC_KEYS = ("ref", "S1", "S2", "m", "r", "cnt")
CYCLIC = (np.array([[-1.1, 1, 0], [0, -1.1, 1], [1, 0, -1.1]]), 0.1 * np.ones(3))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _case(n, N, seed=11):
    """(draw blocks, y, cens, restatement's l[draw, obs]) for bd_exit(n) scaled
    by 0.8 .. 1.25 and N observations, 30 % censored."""
    S, s = bd_exit(n)
    y, cens = simulate_ph(S, s, N, seed=seed, censor_frac=0.3)
    Ss, ss = R.scaled_draws(n)
    blocks = np.stack([P.loglik_block(a, b) for a, b in zip(Ss, ss)])
    return blocks, y, cens, R.pointwise(blocks, y, cens)


def _sweeper(n, y, cens, method=ECS):
    sw = P.Sweeper(n, method, 1, device=0)
    sw.set_obs(y, cens)
    return sw


@pytest.fixture(scope="module")
def case5(gpu):
    return _case(5, 2000)


@pytest.mark.parametrize("n", [3, 5, 7, 10, 15, 20])
def test_pointwise_bit_exact(gpu, n):
    blocks, y, cens, want = _case(n, 2000)
    assert np.all(np.isfinite(want))
    sw = _sweeper(n, y, cens)
    got = sw.loglik_blocks(blocks, pointwise=True)
    sw.close()
    assert np.array_equal(_bits(got["pointwise"]), _bits(want))
    assert np.array_equal(np.stack([got[k] for k in ("H", "F", "nbad", "nobs")], axis=1), R.totals(want))
    assert not got["bad_draw"].any() and np.all(np.isfinite(got["total"]))


@pytest.mark.parametrize("method", [1, 4])
def test_any_method_context(gpu, case5, method):
    """DCS keeps its observations in another order than ECS / MHRS; the
    pointwise values come back in the caller's order from each."""
    blocks, y, cens, want = case5
    sw = _sweeper(5, y, cens, method)
    got = sw.loglik_blocks(blocks, pointwise=True)["pointwise"]
    sw.close()
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_shapes_and_batches(gpu, N):
    n = 5
    blocks, y, cens, want = _case(n, N, seed=12)
    tot = R.totals(want)
    st = R.waic_state(want)
    sw = _sweeper(n, y, cens)
    for batch in (1, 2, 5, 64):
        sw.waic_reset()
        got = sw.loglik_blocks(blocks, batch=batch, accumulate=True)
        assert np.array_equal(np.stack([got[k] for k in ("H", "F", "nbad", "nobs")], axis=1), tot), batch
        gst = sw.waic_state()
        for k in WAIC_KEYS:
            assert np.array_equal(gst[k], st[k]) and np.array_equal(_bits(gst[k].astype(np.float64)),
                                                                    _bits(st[k].astype(np.float64))), (batch, k)
        pw = sw.loglik_blocks(blocks, batch=batch, pointwise=True)["pointwise"]
        assert np.array_equal(_bits(pw), _bits(want)), batch
    sw.close()


def test_shards_add_to_the_whole(gpu, case5):
    blocks, y, cens, want = case5
    words = []
    for lo, hi in ((0, 2000), (0, 777), (777, 2000)):
        sw = _sweeper(5, y[lo:hi], cens[lo:hi])
        r = sw.loglik_blocks(blocks)
        sw.close()
        words.append(np.stack([r[k] for k in ("H", "F", "nbad", "nobs")], axis=1))
    assert np.array_equal(words[1] + words[2], words[0])
    assert np.array_equal(words[0], R.totals(want))


def test_cyclic_draw_in_a_batch(gpu):
    n = 3
    blocks, y, cens, want = _case(n, 2000)
    cyc = P.loglik_block(*CYCLIC)
    assert cyc[:8].view(np.uint64)[0] != 0
    mixed = np.stack([blocks[0], blocks[1], cyc, blocks[2], blocks[3]])
    sw = _sweeper(n, y, cens)
    clean = sw.loglik_blocks(blocks[:4])
    sw.waic_reset()
    got = sw.loglik_blocks(mixed, pointwise=True, accumulate=True)
    st = sw.waic_state()
    sw.close()
    assert got["bad_draw"].tolist() == [False, False, True, False, False]
    assert np.isnan(got["total"][2]) and np.all(np.isfinite(got["total"][[0, 1, 3, 4]]))
    assert np.all(np.isnan(got["pointwise"][2]))
    for k in ("H", "F", "nbad", "nobs"):
        assert got[k][2] == 0
        assert np.array_equal(got[k][[0, 1, 3, 4]], clean[k]), k
    assert np.all(st["cnt"] == 4)
    want_st = R.waic_state(want[:4])
    for k in WAIC_KEYS:
        assert np.array_equal(st[k], want_st[k]), k


def test_accumulate_across_calls_and_waic(gpu, case5):
    from scipy.special import logsumexp

    blocks, y, cens, want = case5
    sw = _sweeper(5, y, cens)
    sw.waic_reset()
    sw.loglik_blocks(blocks, accumulate=True)
    one = sw.waic_state()
    sw.waic_reset()
    sw.loglik_blocks(blocks[:3], accumulate=True)
    sw.loglik_blocks(blocks[3:], accumulate=True)
    two = sw.waic_state()
    pw = sw.loglik_blocks(blocks, pointwise=True)["pointwise"]
    sw.close()
    for k in WAIC_KEYS:
        assert np.array_equal(one[k], two[k]), k
    w = P.waic_from_state(two)
    lppd_i = logsumexp(pw, axis=0) - np.log(5)
    p_i = np.var(pw, axis=0, ddof=1)
    assert np.all(np.abs(w["pointwise"][0] - lppd_i) <= 1e-12 * np.maximum(1, np.abs(lppd_i)))
    assert np.all(np.abs(w["pointwise"][1] - p_i) <= 1e-12 * np.maximum(1, np.abs(p_i)))
    for key, ref in (("lppd", lppd_i.sum()), ("p_waic", p_i.sum()), ("waic", -2 * (lppd_i.sum() - p_i.sum()))):
        assert abs(w[key] - ref) <= 1e-12 * len(y) * max(1, abs(ref)), key


def test_end_to_end_chain(gpu):
    n, N, it = 4, 2000, 12
    S, s = bd_exit(n)
    y, cen = simulate_ph(S, s, N, seed=42, censor_frac=0.3)
    zexp = P.zexp_for(y)
    T, theta = bd_exit_structure(n)
    nu, zeta = 1 + 50 * theta, np.full(len(theta), 50.0)
    Cm = np.ones(T.shape)

    def chain(with_loglik):
        P.set_seed(1)
        sw = _sweeper(n, y, cen)
        if with_loglik:
            sw.loglik([S], [s], accumulate=True)
        res = sw.gibbs(it, ECS, nu, zeta, T, Cm, zexp)
        if with_loglik:
            sw.loglik([S], [s], pointwise=True)
        sw.close()
        return res

    res = chain(True)
    assert np.array_equal(_bits(res), _bits(chain(False)))
    ll = P.log_lik(res, y, T, censored=cen, C_=Cm)
    assert ll.shape == (it,) and np.all(np.isfinite(ll))
    sw = _sweeper(n, y, cen)
    for k in (0, 5, it - 1):
        Sk, sk = P.theta_to_S(res[k], T, Cm)
        assert sw.loglik([Sk], [sk])["total"][0] == ll[k], k
    sw.close()
    w = P.waic(res, y, T, censored=cen, C_=Cm, burn=2)
    assert w["n_draws_used"] == it - 2 and np.isfinite(w["waic"]) and w["p_waic"] > 0


def test_ph_curves(gpu):
    n = 5
    Ss, ss = R.scaled_draws(n, (0.9, 1.0, 1.1))
    T, theta = bd_exit_structure(n)
    draws = np.stack([theta * c for c in (0.9, 1.0, 1.1)])
    grid = np.concatenate([[1e-9], np.linspace(0.05, 8.0, 32)])
    out = P.ph_curves(draws, T, grid)
    assert out["logdens"].shape == out["logsurv"].shape == out["hazard"].shape == (3, 33)
    assert np.array_equal(out["hazard"], np.exp(out["logdens"] - out["logsurv"]))
    assert np.all(np.diff(out["logsurv"], axis=1) <= 0)
    for d in range(3):
        assert abs(out["logdens"][d, 0] - np.log(ss[d][0])) <= 1e-8


def test_no_observations_is_an_error(gpu, lib):
    sw = P.Sweeper(3, ECS, 1, device=0)
    S, s = bd_exit(3)
    with pytest.raises(P.PhaseTypeError, match="no observations"):
        sw.loglik([S], [s])
    assert b"no observations" in lib.pht_last_error()
    with pytest.raises(P.PhaseTypeError, match="no observations"):
        sw.waic_state()
    sw.close()
