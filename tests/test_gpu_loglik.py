"""GPU: the log-likelihood kernel (phasetype_amd/csrc/pht_loglik.hip) against
the CPU restatement of include/pht_loglik.h (tests/loglik_spec.c) bit for
bit: pointwise values, the int64 totals words, the WAIC state; batching,
sharding and partial waves; flagged draws; the Python API end to end.  Off
BD-exit (tests/evaluator_cases.py): the cancellation guard's flag and bad
observations bit for bit, evaluator="auto" on a shared-rate chain and on a
draw with a bad observation, and nothing else moved by such calls."""
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
from phasetype_amd.synth import bd_exit, bd_exit_structure, simulate_ph  # noqa: E402

pytestmark = pytest.mark.gpu

ECS = 2
WAIC_KEYS = ("ref", "S1", "S2", "m", "r", "cnt")
CYCLIC = (np.array([[-1.1, 1, 0], [0, -1.1, 1], [1, 0, -1.1]]), 0.1 * np.ones(3))
SCALES = (0.8, 0.9, 1.0, 1.1, 1.25)


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


def _same_nan_and_bits(got, want):
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(_bits(np.nan_to_num(got, nan=0.0)),
                                                                            _bits(np.nan_to_num(want, nan=0.0)))


def off_bd_draws(family, n):
    """(S_list, s_list, y, cens): the family's generator scaled by 0.8 .. 1.25
    (nearly equal rates 1e-3 apart: at n = 3 a usable block with accepted and
    rejected observations) and 65 observations, one wavefront plus one: the
    grid of tests/evaluator_cases.py, exact and censored interleaved"""
    S, s = EC.generator(family, n, **({"eps": 1e-3} if family == "gapped" else {}))
    Ss, ss = [S * c for c in SCALES], [s * c for c in SCALES]
    y, cens = EC.tiled(*EC.observations(S, scale=max(SCALES)), 65)
    return Ss, ss, y, cens


@pytest.mark.parametrize("n", EC.NEW_N)
@pytest.mark.parametrize("family", EC.FAMILIES)
def test_pointwise_bit_exact_off_bd_exit(gpu, family, n):
    """The kernel against the restatement off BD-exit, guard included: the
    compile-time-n kernels (n = 3, 10) and the runtime-n one (n = 6), batch 1
    and 64, totals-only and pointwise.  Flagged draws, accepted and rejected
    observations share a launch and a wavefront."""
    Ss, ss, y, cens = off_bd_draws(family, n)
    blocks = np.stack([P.loglik_block(a, b) for a, b in zip(Ss, ss)])
    flags = np.ascontiguousarray(blocks[:, :8]).view(np.uint64).reshape(-1)
    want = R.pointwise(blocks, y, cens)
    tot = R.totals(want)
    tot[flags != 0] = 0
    assert np.all(np.isnan(want[flags != 0]))
    if family in ("erlang", "coxian_shared"):
        assert np.all(flags & np.uint64(P.LL_F_ILLCOND))
    if family in ("bd", "reversible"):
        assert not flags.any() and np.all(np.isfinite(want[:, y >= 1e-3]))
    sw = _sweeper(n, y, cens)
    for batch in (1, 64):
        got = sw.loglik_blocks(blocks, batch=batch)
        assert np.array_equal(np.stack([got[k] for k in ("H", "F", "nbad", "nobs")], axis=1), tot), batch
        assert np.array_equal(got["bad_draw"], flags != 0)
        got = sw.loglik_blocks(blocks, batch=batch, pointwise=True)
        assert _same_nan_and_bits(got["pointwise"], want), batch
        assert np.array_equal(np.stack([got[k] for k in ("H", "F", "nbad", "nobs")], axis=1), tot), batch
        assert np.array_equal(np.isnan(got["total"]), flags != 0)
        assert np.array_equal(np.isneginf(got["total"]), (flags == 0) & (tot[:, 2] > 0))
    sw.close()


def _erlang_structure(n):
    """T of the chain 1 -> 2 -> ... -> n -> absorbed with ONE variable on
    every transition: every draw is Erlang(n, theta), exactly defective"""
    T = np.zeros((n + 1, n + 1), np.int32)
    for i in range(n):
        T[i, i + 1] = 1
    return T


def test_auto_on_a_shared_rate_chain(gpu):
    """A structure that names one variable on every transition: under the
    default evaluator every draw is flagged ILLCOND and NaN; under "auto"
    every draw goes to uniformisation, totals and WAIC state bit-equal to
    evaluator="unif"; the PSIS-LOO matrix has no NaN row."""
    n, it, N = 4, 12, 257
    T = _erlang_structure(n)
    S, s = EC.erlang(n)
    y, cen = simulate_ph(S, s, N, seed=21, censor_frac=0.3)
    rows = EC.LAM * np.linspace(0.8, 1.25, it)[:, None]  # the chain's draws: one column
    draws = [P.theta_to_S(r, T) for r in rows]
    Ss, ss = [d[0] for d in draws], [d[1] for d in draws]
    assert np.array_equal(Ss[3], EC.erlang(n, rows[3, 0])[0])
    flags = np.array([P.loglik_block(a, b)[:8].view(np.uint64)[0] for a, b in zip(Ss, ss)])
    assert np.all(flags & np.uint64(P.LL_F_ILLCOND)) and not np.any(flags & np.uint64(P.LL_F_NONFINITE))
    assert np.all(np.isnan(P.log_lik(rows, y, T, censored=cen)))
    sw = _sweeper(n, y, cen)
    dflt = sw.loglik(Ss, ss, pointwise=True)
    assert dflt["bad_draw"].all() and np.all(np.isnan(dflt["total"])) and np.all(np.isnan(dflt["pointwise"]))
    sw.waic_reset()
    unif = sw.loglik(Ss, ss, accumulate=True, evaluator="unif")
    st_unif = sw.waic_state()
    sw.waic_reset()
    auto = sw.loglik(Ss, ss, accumulate=True, evaluator="auto")
    st_auto = sw.waic_state()
    loo = sw.psis_loo(Ss, ss, evaluator="auto")
    sw.close()
    assert auto["evaluator"].tolist() == ["unif"] * it
    assert np.all(np.isfinite(auto["total"])) and np.array_equal(_bits(auto["total"]), _bits(unif["total"]))
    for k in ("H", "F", "nbad", "nobs"):
        assert np.array_equal(auto[k], unif[k]), k
    assert np.all(st_auto["cnt"] == it)
    for k in WAIC_KEYS:
        assert np.array_equal(_bits(st_auto[k].astype(np.float64)), _bits(st_unif[k].astype(np.float64))), k
    assert loo["evaluator"].tolist() == ["unif"] * it and not loo["bad_draw"].any()
    assert loo["n_draws_used"] == it and not np.any(loo["flags"] & 1), "no NaN row in the matrix"
    assert np.array_equal(_bits(loo["total"]), _bits(unif["total"]))
    assert np.array_equal(_bits(P.log_lik(rows, y, T, censored=cen, evaluator="auto")), _bits(unif["total"]))
    assert P.loo(rows, y, T, censored=cen, evaluator="auto")["n_draws_used"] == it


def test_auto_reroutes_a_draw_with_a_bad_observation(gpu):
    """hypoexp(3) is well conditioned (flag 0) but at y = 1e-9 its density sum
    cancels past the guard: the default total is -inf, "auto" finds the draw
    in its totals-only pass and evaluates it by uniformisation, once, in draw
    order."""
    n = 3
    bdS, bds = bd_exit(n)
    hS, hs = EC.hypoexp(n)
    Ss, ss = [bdS, hS, 1.1 * bdS, 0.9 * hS], [bds, hs, 1.1 * bds, 0.9 * hs]
    mu = max(float(np.max(-np.diag(a))) for a in Ss)
    y, cens = EC.tiled(*EC.observations(hS, scale=mu / float(np.max(-np.diag(hS)))), 65)
    blocks = np.stack([P.loglik_block(a, b) for a, b in zip(Ss, ss)])
    assert not np.ascontiguousarray(blocks[:, :8]).view(np.uint64).any()
    mixed = R.pointwise(blocks, y, cens)
    assert np.all(np.isfinite(mixed[[0, 2]])) and np.isnan(mixed[[1, 3]]).any()
    mixed[[1, 3]] = U.pointwise([Ss[1], Ss[3]], [ss[1], ss[3]], y, cens)
    assert np.all(np.isfinite(mixed))
    sw = _sweeper(n, y, cens)
    dflt = sw.loglik(Ss, ss, blocks=blocks)
    sw.waic_reset()
    got = sw.loglik(Ss, ss, pointwise=True, accumulate=True, evaluator="auto", blocks=blocks)
    st = sw.waic_state()
    sw.close()
    assert np.isneginf(dflt["total"]).tolist() == [False, True, False, True] and (dflt["nbad"] > 0).tolist() == [
        False, True, False, True]
    assert got["evaluator"].tolist() == ["spectral", "unif", "spectral", "unif"]
    assert np.array_equal(_bits(got["pointwise"]), _bits(mixed)) and np.all(got["nbad"] == 0)
    want_st = R.waic_state(mixed)
    assert np.all(st["cnt"] == 4)
    for k in WAIC_KEYS:
        assert np.array_equal(_bits(st[k].astype(np.float64)), _bits(want_st[k].astype(np.float64))), k


def test_nothing_else_moves(gpu):
    """The chain and the WAIC state of a bd_exit(5) run are bit-identical with
    and without interleaved ill-conditioned calls (flagged under the default
    evaluator, rerouted under "auto")."""
    n, N, it = 5, 1000, 6
    S, s = bd_exit(n)
    eS, es = EC.erlang(n)
    y, cen = simulate_ph(S, s, N, seed=43, censor_frac=0.3)
    zexp = P.zexp_for(y)
    T, theta = bd_exit_structure(n)
    nu, zeta = 1 + 50 * theta, np.full(len(theta), 50.0)
    Cm = np.ones(T.shape)
    Ss, ss = R.scaled_draws(n)

    def run(interleave):
        P.set_seed(1)
        sw = _sweeper(n, y, cen)
        sw.waic_reset()
        sw.loglik(Ss[:2], ss[:2], accumulate=True)
        if interleave:
            r = sw.loglik([eS, 1.1 * eS], [es, 1.1 * es], accumulate=True)  # flagged: nothing to accumulate
            assert r["bad_draw"].all()
            r = sw.loglik([eS], [es], pointwise=True, evaluator="auto")
            assert r["evaluator"].tolist() == ["unif"] and np.isfinite(r["total"][0])
        a = sw.gibbs(it, ECS, nu, zeta, T, Cm, zexp)
        if interleave:
            sw.psis_loo([eS, S], [es, s], evaluator="auto")
        sw.loglik(Ss[2:], ss[2:], accumulate=True, evaluator="auto")
        b = sw.gibbs(it, ECS, nu, zeta, T, Cm, zexp, start=a[-1])
        st = sw.waic_state()
        sw.close()
        return np.concatenate([a, b]), st

    res0, st0 = run(False)
    res1, st1 = run(True)
    assert np.array_equal(_bits(res0), _bits(res1))
    assert np.all(st0["cnt"] == 5)
    for k in WAIC_KEYS:
        assert np.array_equal(_bits(st0[k].astype(np.float64)), _bits(st1[k].astype(np.float64))), k


def test_no_observations_is_an_error(gpu, lib):
    sw = P.Sweeper(3, ECS, 1, device=0)
    S, s = bd_exit(3)
    with pytest.raises(P.PhaseTypeError, match="no observations"):
        sw.loglik([S], [s])
    assert b"no observations" in lib.pht_last_error()
    with pytest.raises(P.PhaseTypeError, match="no observations"):
        sw.waic_state()
    sw.close()
