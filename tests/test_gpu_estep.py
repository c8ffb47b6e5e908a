"""GPU: the E-step kernels (phasetype_amd/csrc/pht_estep.hip) against the
tests' restatement of include/pht_estep.h (tests/estep_spec.c), bit for bit;
integer equality across batch, grid and shards; no interference with the
log-likelihood and the sampler; ph_em on the GPU; the samplers' sweep means
against the exact expectations."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import estep_ref as R  # noqa: E402
import evaluator_cases as EC  # noqa: E402
import loglik_unif_ref as U  # noqa: E402
import phasetype_amd as P  # noqa: E402
from phasetype_amd.synth import bd_exit, simulate_ph  # noqa: E402

pytestmark = pytest.mark.gpu

ECS, UNIF = 2, 8
KEYS = ("Z", "N", "E", "A")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _gen(n):
    return {1: (np.array([[-0.7]]), np.array([0.7])), 3: U.CYCLIC}.get(n) or bd_exit(n)


def _case(n, N, nd, seed=21):
    """nd draws (the generator scaled by 0.8 .. 1.25; with three or more, draw
    1 carries a NaN) and exactly N observations, 30 % censored: simulated ones,
    and from N = 63 on the edge y's (each exact and censored) and one y with
    mu y >= 2047 for every draw (bad: counted, not added)."""
    S, s = _gen(n)
    scales = np.linspace(0.8, 1.25, nd) if nd > 1 else np.array([1.0])
    Ss, ss = [S * c for c in scales], [s * c for c in scales]
    if nd >= 3:
        Ss[1] = Ss[1].copy()
        Ss[1][0, 0] = np.nan
    extra = 7 if N >= 63 else 0
    y, cens = simulate_ph(S, s, N - extra, seed=seed, censor_frac=0.3)
    if extra:
        y, cens = U.with_edges(y, cens)
        y = np.concatenate([y, [2100.0 / (0.8 * np.max(-np.diag(S)))]])
        cens = np.concatenate([cens, [0]]).astype(np.int32)
    assert len(y) == N
    return Ss, ss, y, cens


def _want(Ss, ss, y, cens, yscale=None, ymax=None):
    return [R.estep(S, s, y, cens, yscale=yscale, ymax=ymax) for S, s in zip(Ss, ss)]


def _sweeper(n, y, cens, method=ECS):
    sw = P.Sweeper(n, method, 1, device=0)
    sw.set_obs(y, cens)
    return sw


def _check(got, want, tag=None):
    for d, w in enumerate(want):
        assert int(got["flags"][d]) == w["flag"], (tag, d)
        assert np.array_equal(got["words"][d], w["words"]), (tag, d)
        assert [int(got[k][d]) for k in ("H", "F", "nbad", "nobs")] == [int(v) for v in w["totals"]], (tag, d)
        for k in KEYS:
            assert np.array_equal(_bits(got[k][d]), _bits(w[k])), (tag, d, k)
        assert np.array_equal(_bits(got["loglik"][d]), _bits(w["loglik"])), (tag, d)


@pytest.mark.parametrize("n,N,nd", [(1, 1, 1), (3, 63, 3), (10, 513, 65), (32, 1100, 3), (3, 1100, 65), (10, 1, 3),
                                    (32, 63, 1), (1, 513, 3)])
def test_bit_equal_to_the_restatement(gpu, n, N, nd):
    Ss, ss, y, cens = _case(n, N, nd)
    want = _want(Ss, ss, y, cens)
    if N >= 63:
        assert all(w["nbad"] == 1 for w in want if w["flag"] == 0)
    if nd >= 3:
        assert want[1]["flag"] == P.LL_F_NONFINITE and not want[1]["words"].any()
    sw = _sweeper(n, y, cens)
    got = sw.estep(Ss, ss)
    sw.close()
    assert got["yscale"] == want[0]["yscale"]
    _check(got, want, (n, N, nd))


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


@pytest.mark.parametrize("case", EC.OFF_BD_GPU, ids=EC.case_id)
def test_off_bd_exit_bit_equal_to_the_restatement(gpu, sweepers, case):
    """The families of tests/evaluator_cases.py through the histogram and the
    contraction: rows of R with one non-zero, forward vectors with exact
    zeros, a shift for R (Erlang), rates over four decades (stiff).  5 draws,
    130 observations (the grid of y, each exact and censored, tiled; ties),
    batch 64 and 2; no draw flagged, no observation bad, every value finite,
    in the restatement and on the GPU."""
    family, n, kw = case
    S, s = EC.generator(family, n, **kw)
    Ss, ss = U.scaled(S, s)
    y, cens = EC.tiled(*EC.observations(S, scale=EC.DRAW_SCALE), 130)
    want = _want(Ss, ss, y, cens)
    for w in want:
        assert w["flag"] == 0 and w["nbad"] == 0 and int(w["totals"][3]) == 130 and np.isfinite(w["loglik"])
        assert all(np.all(np.isfinite(w[k])) for k in KEYS)
    sw = sweepers(n)
    sw.set_obs(y, cens)
    for batch in (64, 2):
        got = sw.estep(Ss, ss, batch=batch)
        assert got["yscale"] == want[0]["yscale"]
        assert not np.asarray(got["flags"]).any() and not np.asarray(got["nbad"]).any()
        assert np.all(np.asarray(got["nobs"]) == 130) and np.all(np.isfinite(got["loglik"]))
        assert all(np.all(np.isfinite(got[k])) for k in KEYS)
        _check(got, want, (EC.case_id(case), batch))


@pytest.fixture(scope="module")
def case10(gpu):
    Ss, ss, y, cens = _case(10, 1100, 5)
    return Ss, ss, y, cens, _want(Ss, ss, y, cens)


def test_integers_do_not_depend_on_batch_or_grid(gpu, case10):
    Ss, ss, y, cens, want = case10
    sw = _sweeper(10, y, cens)
    for batch, cap in ((1, 0), (2, 0), (64, 0), (64, 1), (3, 2)):
        _check(sw.estep(Ss, ss, batch=batch, grid_cap=cap), want, (batch, cap))
    h = sw.estep(Ss, ss, contract=False)
    sw.close()
    assert h["Z"] is None and all(np.array_equal(h["words"][d], w["words"]) for d, w in enumerate(want))


def test_two_shards_with_a_common_yscale(gpu, case10):
    Ss, ss, y, cens, want = case10
    ys = want[0]["yscale"]
    parts = []
    for lo, hi in ((0, 400), (400, len(y))):
        sw = _sweeper(10, y[lo:hi], cens[lo:hi])
        parts.append(sw.estep(Ss, ss, yscale=ys, contract=False))
        sw.close()
        ref = _want(Ss, ss, y[lo:hi], cens[lo:hi], yscale=ys)
        assert all(np.array_equal(parts[-1]["words"][d], w["words"]) for d, w in enumerate(ref))
    words = parts[0]["words"] + parts[1]["words"]
    # the bad observation sits in the second shard, whose table alone reaches
    # the cap: the sums still equal the whole's words exactly
    for d, w in enumerate(want):
        assert np.array_equal(words[d], w["words"]), d
        if w["flag"] == 0:
            c = P.estep_contract(Ss[d], ss[d], words[d], ys)
            for k in KEYS:
                assert np.array_equal(_bits(c[k]), _bits(w[k])), (d, k)
    sw = _sweeper(10, y[:400], cens[:400])
    with pytest.raises(P.PhaseTypeError):
        sw.estep(Ss, ss, yscale=2.0 ** -3)  # smaller than an observation
    sw.close()


def test_loglik_is_the_uniformisation_evaluators(gpu, case10):
    Ss, ss, y, cens, want = case10
    sw = _sweeper(10, y, cens)
    a = sw.loglik_unif(Ss, ss)
    b = sw.estep(Ss, ss)
    c = sw.loglik_unif(Ss, ss)
    sw.close()
    for k in ("H", "F", "nbad", "nobs"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    assert np.array_equal(_bits(a["total"]), _bits(b["loglik"]))


def test_unif_sampler_chain_is_untouched(gpu):
    n, it = 3, 6
    T = np.zeros((4, 4), np.int32)
    T[0, 1], T[0, 3], T[1, 2], T[1, 3], T[2, 0], T[2, 3] = 1, 2, 3, 4, 5, 6
    theta = np.array([1.0, 0.1, 1.0, 0.1, 1.0, 0.1])
    S, s = P.theta_to_S(theta, T)
    y, cen = simulate_ph(S, s, 1000, seed=15, censor_frac=0.3)
    nu, zeta, Cm, zexp = 1 + 50 * theta, np.full(len(theta), 50.0), np.ones(T.shape), P.zexp_for(y)

    def chain(with_estep):
        P.set_seed(1)
        sw = _sweeper(n, y, cen, UNIF)
        if with_estep:
            sw.estep([S, 1.1 * S], [s, 1.1 * s])
        a = sw.gibbs(it, UNIF, nu, zeta, T, Cm, zexp)
        if with_estep:
            sw.estep([S], [s], contract=False)
        b = sw.gibbs(it, UNIF, nu, zeta, T, Cm, zexp, start=a[-1])
        sw.close()
        return np.concatenate([a, b])

    assert np.array_equal(_bits(chain(True)), _bits(chain(False)))


def test_ph_em_reproduces_the_restatement(gpu):
    S, s = bd_exit(3)
    x, cens = simulate_ph(S, s, 300, seed=11, censor_frac=0.3)
    T = np.array([[0, 1, 0, 3], [2, 0, 1, 3], [0, 2, 0, 4], [0, 0, 0, 0]], np.int32)
    Cm = np.ones((4, 4))
    Cm[1, 2] = 2.5
    kw = dict(C_=Cm, start=[1.0, 0.7, 0.5, 1.5], iters=30, tol=0.0)
    want = P.ph_em(x, T, cens, estep=lambda S_, s_: R.estep(S_, s_, x, cens), **kw)
    got = P.ph_em(x, T, cens, **kw)
    assert got["iterations"] == 30
    assert np.array_equal(_bits(got["loglik"]), _bits(want["loglik"]))
    assert np.array_equal(_bits(got["theta"]), _bits(want["theta"]))
    # the fit is usable as a chain's start
    sw = _sweeper(3, x, cens)
    P.set_seed(3)
    res = sw.gibbs(3, ECS, 1 + got["theta"], np.ones(4), T, Cm, P.zexp_for(x), start=got["theta"])
    sw.close()
    assert res.shape == (3, 4) and np.all(np.isfinite(res)) and np.all(res > 0)


@pytest.mark.parametrize("method", [ECS, UNIF])
def test_sampler_against_the_exact_expectations(gpu, method):
    """bd_exit(4), N = 2000, 30 % censored, 64 sweeps with distinct keys: every
    cell's sweep mean of z, N and exits within 5 standard errors (from the
    sweep-to-sweep spread; counts floored at the Poisson level, as
    oracle/posterior.py sweep_zscores floors them) of expected_stats.  The
    samplers run a censored path on to absorption (the reference's law), so
    the truth is expected_stats(complete=True): the statistics on [0, y] plus
    what the state occupancy at y implies beyond it.  (On [0, y] alone the
    sampler's sum z exceeds sum y by the censored paths' remainders: 6477
    against 5793 on these inputs.)  The same inputs through the CPU oracle's
    device variant: largest z-score 2.0 (ECS), 3.3 (UNIF)."""
    n, N, sweeps = 4, 2000, 64
    S, s = bd_exit(n)
    rng = np.random.default_rng(7)
    y = rng.gamma(2.0, 1.5, N)
    cens = (rng.random(N) < 0.3).astype(np.int32)
    truth = P.expected_stats(S, s, y, cens, complete=True)
    assert truth["nbad"] == 0 and abs(truth["E"].sum() - N) < 1e-6
    zexp = P.zexp_for(y)
    sw = _sweeper(n, y, cens, method)
    zs, Ns = [], []
    for k in range(sweeps):
        zq, _, Nk, _ = P.split_stats(sw.sweep(S, s, key=(1000 + k, 77), sweep=k + 1, zexp=zexp), n)
        zs.append(zq * 2.0 ** -zexp)
        Ns.append(Nk.astype(np.float64))
    sw.close()
    want_N = truth["N"] + np.diag(truth["E"])  # the block's diagonal counts the exits
    for name, X, want, floor in (("z", np.array(zs), truth["Z"], False), ("N", np.array(Ns), want_N, True)):
        mean, se = X.mean(0), X.std(0, ddof=1) / np.sqrt(sweeps)
        if floor:
            se = np.maximum(se, np.sqrt(want / sweeps))
        d = np.abs(mean - want)
        zsc = np.where(se > 0, d / np.where(se > 0, se, 1.0), np.where(d > 0, np.inf, 0.0))
        print(f"method {method} {name}: largest z-score {zsc.max():.2f}")
        assert np.all(zsc <= 5.0), (method, name, zsc)
