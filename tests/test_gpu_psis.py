"""GPU: the PSIS-LOO kernels (phasetype_amd/csrc/pht_psis.hip) against the CPU
restatement of include/pht_psis.h (tests/psis_spec.c) bit for bit, the
restatement fed the GPU's own pointwise log-likelihoods; draw and observation
counts around the wave and tile sizes; flagged rows skipped; fills in any
split and order; ties, constant tails and bad observations; nothing else on
the context touched; the Python API end to end."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import loglik_unif_ref as U  # noqa: E402
import phasetype_amd as P  # noqa: E402
import psis_ref as R  # noqa: E402
from phasetype_amd.synth import bd_exit, bd_exit_structure, simulate_ph  # noqa: E402

pytestmark = pytest.mark.gpu

ECS = 2
OUT = ("elpd_i", "khat", "lppd_i")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _draws(S0, s0, nd, seed):
    """nd generators around (S0, s0): every rate scaled by c_d, the exit rates
    by e_d as well (two directions, so the draws' l do not order alike)."""
    rng = np.random.default_rng(seed)
    c, e = np.exp(rng.normal(0.0, 0.15, nd)), np.exp(rng.normal(0.0, 0.25, nd))
    off = S0 - np.diag(np.diag(S0))
    Ss, ss = [], []
    for cd, ed in zip(c, e):
        s = s0 * cd * ed
        A = off * cd
        Ss.append(A - np.diag(A.sum(axis=1) + s))
        ss.append(s)
    return Ss, ss


def _same(got, want, tag=None):
    for k in OUT:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (tag, k, got[k], want[k])
    assert np.array_equal(got["flags"], want["flags"]), (tag, got["flags"], want["flags"])
    assert got["n_draws_used"] == want["n_draws_used"], tag
    assert np.array_equal(_bits(got["p_loo_i"]), _bits(got["lppd_i"] - got["elpd_i"])), tag


def _sweeper(n, y, cens):
    sw = P.Sweeper(n, ECS, 1, device=0)
    sw.set_obs(y, cens)
    return sw


@pytest.fixture(scope="module")
def pool(gpu):
    """per n: 4096 draws with their spectral blocks, computed once"""
    out = {}
    for n in (3, 10):
        S0, s0 = bd_exit(n)
        Ss, ss = _draws(S0, s0, 4096, seed=40 + n)
        out[n] = (S0, s0, Ss, ss, np.stack([P.loglik_block(a, b) for a, b in zip(Ss, ss)]))
    return out


@pytest.mark.parametrize("S", [24, 25, 63, 64, 65, 400, 1000, 4096])
@pytest.mark.parametrize("n", [3, 10])
def test_bit_exact_against_the_restatement(gpu, pool, n, S):
    S0, s0, Ss, ss, blocks = pool[n]
    Ss, ss, blocks = Ss[:S], ss[:S], blocks[:S]
    for N in (1, 63, 64, 65, 300):
        y, cens = simulate_ph(S0, s0, N, seed=100 + N, censor_frac=0.3)
        sw = _sweeper(n, y, cens)
        ll = sw.loglik(Ss, ss, pointwise=True, blocks=blocks)
        got = sw.psis_loo(Ss, ss, blocks=blocks)
        sw.close()
        assert not ll["bad_draw"].any() and np.all(np.isfinite(ll["pointwise"]))
        want = R.psis(ll["pointwise"])
        _same(got, want, (n, S, N))
        assert np.array_equal(_bits(got["total"]), _bits(ll["total"]))
        assert np.all(got["flags"] == (R.F_SHORT if S < 25 else 0)), (S, N, got["flags"])
        assert np.all(np.isfinite(got["khat"]) == (S >= 25))


def test_cyclic_structure_and_skipped_rows(gpu):
    n = 5
    S0, s0 = bd_exit(n)
    Sr, sr = U.ring(n)
    Ss, ss = _draws(S0, s0, 60, seed=50)
    Sc, sc = _draws(Sr, sr, 60, seed=51)
    cyc = np.zeros(60, bool)
    cyc[10:20] = cyc[40:45] = True
    Ss = [Sc[d] if cyc[d] else Ss[d] for d in range(60)]
    ss = [sc[d] if cyc[d] else ss[d] for d in range(60)]
    y, cens = simulate_ph(S0, s0, 130, seed=52, censor_frac=0.3)
    sw = _sweeper(n, y, cens)
    for ev in ("unif", "auto", "spectral"):
        ll = sw.loglik(Ss, ss, pointwise=True, evaluator=ev)
        got = sw.psis_loo(Ss, ss, evaluator=ev, batch=7)
        assert np.array_equal(got["bad_draw"], cyc if ev == "spectral" else np.zeros(60, bool)), ev
        assert np.array_equal(got["bad_draw"], ll["bad_draw"]) and np.array_equal(got["evaluator"], ll["evaluator"])
        assert np.array_equal(_bits(got["total"]), _bits(ll["total"])), ev
        want = R.psis(ll["pointwise"], ~ll["bad_draw"])
        _same(got, want, ev)
        assert got["n_draws_used"] == (45 if ev == "spectral" else 60)
        assert np.all(got["flags"] == 0)
    sw.close()


def test_fill_splits_orders_and_batches(gpu, pool):
    n, S = 10, 200
    S0, s0, Ss, ss, blocks = pool[n]
    Ss, ss, blocks = Ss[:S], ss[:S], blocks[:S]
    y, cens = simulate_ph(S0, s0, 150, seed=60, censor_frac=0.3)
    sw = _sweeper(n, y, cens)
    whole = sw.psis_loo(Ss, ss, blocks=blocks)
    for batch, cuts in ((1, (0, 120, 200)), (7, (0, 33, 150, 200)), (64, (0, 65, 129, 200))):
        sw.loo_begin(S)
        tot = np.zeros((S, 4), np.int64)
        spans = list(zip(cuts[:-1], cuts[1:]))[::-1]  # the last rows first
        for lo, hi in spans:
            tot[lo:hi], bad = sw.loo_fill(lo, blocks=blocks[lo:hi], batch=batch)
            assert not bad.any()
        got = sw.loo_result()
        sw.loo_end()
        _same(got, whole, (batch, cuts))
        assert np.array_equal(_bits(P.loglik_total(tot[:, 0], tot[:, 1], tot[:, 2], np.zeros(S, bool))),
                              _bits(whole["total"]))
    # rows never filled stay unusable
    sw.loo_begin(S)
    sw.loo_fill(100, blocks=blocks[100:160])
    got = sw.loo_result()
    sw.loo_end()
    _same(got, R.psis(sw.loglik(Ss[100:160], ss[100:160], pointwise=True, blocks=blocks[100:160])["pointwise"]))
    sw.close()


def test_ties_and_constant_tail_from_duplicated_draws(gpu, pool):
    n = 3
    S0, s0, Ss, ss, blocks = pool[n]
    y, cens = simulate_ph(S0, s0, 70, seed=61, censor_frac=0.3)
    sw = _sweeper(n, y, cens)
    # 32 draws four times each: S = 128, M = 25 = 6 x 4 + 1, so the cutoff ties with a tail value
    idx = np.tile(np.arange(32), 4)
    for order in (idx, np.sort(idx), idx[::-1]):
        b = blocks[order]
        ll = sw.loglik([Ss[d] for d in order], [ss[d] for d in order], pointwise=True, blocks=b)
        got = sw.psis_loo([Ss[d] for d in order], [ss[d] for d in order], blocks=b)
        _same(got, R.psis(ll["pointwise"]))
        assert np.all((got["flags"] == 0) | (got["flags"] == R.F_FIT))
        assert np.array_equal(np.isfinite(got["khat"]), got["flags"] == 0)
    same = [0] * 100
    got = sw.psis_loo([Ss[d] for d in same], [ss[d] for d in same], blocks=blocks[same])
    ll = sw.loglik([Ss[0]], [ss[0]], pointwise=True, blocks=blocks[:1])
    sw.close()
    _same(got, R.psis(np.tile(ll["pointwise"], (100, 1))))
    assert np.all(got["flags"] == R.F_CONST) and np.all(np.isposinf(got["khat"]))


def test_an_observation_bad_for_one_usable_draw(gpu):
    n = 5
    S, s = U.ring(n)
    y, cens = simulate_ph(S, s, 100, seed=62, censor_frac=0.3)
    y2, cens2 = np.append(y, 1.5 * y.max()), np.append(cens, 0).astype(np.int32)
    big = 1500.0 / (4.0 * y.max())  # mu y_max = 1500: the appended observation is beyond this draw's table
    rng = np.random.default_rng(63)
    scales = list(np.exp(rng.normal(0.0, 0.1, 40)))
    scales[13] = big
    Ss, ss = U.scaled(S, s, scales)
    sw = _sweeper(n, y2, cens2)
    ll = sw.loglik(Ss, ss, pointwise=True, evaluator="unif")
    got = sw.psis_loo(Ss, ss, evaluator="unif")
    sw.close()
    assert not ll["bad_draw"].any() and np.isnan(ll["pointwise"][13, -1]) and np.isfinite(ll["pointwise"][:, :-1]).all()
    _same(got, R.psis(ll["pointwise"]))
    assert got["flags"][-1] == R.F_BAD and all(np.isnan(got[k][-1]) for k in OUT)
    assert np.all(got["flags"][:-1] == 0) and np.isneginf(got["total"][13])


def test_nothing_else_on_the_context_is_touched(gpu):
    n, it = 3, 6
    T, theta = bd_exit_structure(3)
    S, s = P.theta_to_S(theta, T)
    y, cen = simulate_ph(S, s, 1000, seed=15, censor_frac=0.3)
    nu, zeta, Cm, zexp = 1 + 50 * theta, np.full(len(theta), 50.0), np.ones(T.shape), P.zexp_for(y)
    Ss, ss = _draws(S, s, 40, seed=64)

    def run(with_loo):
        P.set_seed(1)
        sw = P.Sweeper(n, ECS, 1, device=0)
        sw.set_obs(y, cen)
        sw.waic_reset()
        l0 = sw.loglik(Ss[:20], ss[:20], accumulate=True)
        if with_loo:
            r = sw.psis_loo(Ss, ss)
            assert np.all(r["flags"] == 0)
        a = sw.gibbs(it, ECS, nu, zeta, T, Cm, zexp)
        if with_loo:
            sw.psis_loo(Ss, ss, evaluator="unif", batch=3)
        l1 = sw.loglik(Ss[20:], ss[20:], accumulate=True)
        b = sw.gibbs(it, ECS, nu, zeta, T, Cm, zexp, start=a[-1])
        st = sw.waic_state()
        sw.close()
        return np.concatenate([a, b]), np.concatenate([l0["total"], l1["total"]]), st

    c1, t1, st1 = run(True)
    c0, t0, st0 = run(False)
    assert np.array_equal(_bits(c1), _bits(c0)) and np.array_equal(_bits(t1), _bits(t0))
    for k in ("ref", "S1", "S2", "m", "r"):
        assert np.array_equal(_bits(st1[k]), _bits(st0[k])), k
    assert np.array_equal(st1["cnt"], st0["cnt"]) and np.all(st0["cnt"] == 40)


def test_limits_error_cleanly(gpu):
    S, s = bd_exit(3)
    sw = P.Sweeper(3, ECS, 1, device=0)
    with pytest.raises(P.PhaseTypeError, match="no observations"):
        sw.loo_begin(100)
    sw.set_obs(np.array([0.5, 1.0, 2.0]))
    for nd in (0, 16385):
        with pytest.raises(P.PhaseTypeError, match="thin the chain"):
            sw.loo_begin(nd)
    with pytest.raises(P.PhaseTypeError, match="pht_ctx_loo_begin"):
        sw.loo_result()
    blk = P.loglik_block(S, s)[None, :]
    with pytest.raises(P.PhaseTypeError, match="pht_ctx_loo_begin"):
        sw.loo_fill(0, blocks=blk)
    sw.loo_begin(4)
    with pytest.raises(P.PhaseTypeError, match="outside the matrix"):
        sw.loo_fill(4, blocks=blk)
    with pytest.raises(P.PhaseTypeError, match="no usable draw"):
        sw.loo_result()
    sw.loo_fill(3, blocks=blk)
    assert sw.loo_result()["n_draws_used"] == 1
    sw.loo_end()
    # the context still serves: a whole run after the refusals
    r = sw.psis_loo([S] * 30, [s] * 30)
    sw.close()
    assert np.all(r["flags"] == R.F_CONST)


def test_end_to_end_loo_of_a_chain(gpu):
    S, s = bd_exit(3)
    x, _ = simulate_ph(S, s, 500, seed=21)
    TT = np.array([["0", "f1", "0", "e1"], ["b1", "0", "f2", "e2"], ["0", "b2", "0", "e3"], ["0", "0", "0", "0"]],
                  dtype=object)
    truth = dict(f1=2.0, f2=2.0, b1=0.5, b2=0.5, e1=0.3, e2=0.3, e3=2.0)
    P.set_seed(7)
    res = P.phtMCMC2(x, TT, [1, 0, 0], {k: 1 + 50 * v for k, v in truth.items()}, {k: 50.0 for k in truth}, 200,
                     silent=True)
    a = P.loo(res, x, burn=20, evaluator="auto")
    w = P.waic(res, x, burn=20, evaluator="auto")
    print(f"elpd_loo {a['elpd_loo']:.4f} p_loo {a['p_loo']:.4f} p_waic {w['p_waic']:.4f} "
          f"largest khat {np.max(a['pointwise'][2]):.3f} threshold {a['khat_threshold']:.3f}")
    assert a["n_draws_used"] == w["n_draws_used"] == 180
    assert np.isfinite(a["elpd_loo"]) and a["looic"] == -2.0 * a["elpd_loo"]
    assert abs(a["lppd"] - w["lppd"]) <= 1e-9 * abs(w["lppd"])
    assert abs(a["p_loo"] - w["p_waic"]) <= 0.5
    b = P.loo(res, x, burn=20, thin=2, evaluator="auto")
    assert b["n_draws_used"] == 90
    c = P.loo_compare(a, b)
    assert np.isfinite(c["elpd_diff"]) and c["se_diff"] >= 0.0
