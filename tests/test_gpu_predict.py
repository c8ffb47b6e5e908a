"""GPU: the posterior-predictive kernel (phasetype_amd/csrc/pht_predict.hip)
against the CPU restatement of include/pht_predict.h (tests/predict_spec.c) bit
for bit: pointwise values, jump counts, the int64 words, the histogram and the
extremes; every shape of grid, batch and replicate split; long divergent paths;
flags, horizon and jump cap; the samplers' chains and the log-likelihood
untouched; the Python API end to end."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import evaluator_cases as EC  # noqa: E402
import loglik_unif_ref as U  # noqa: E402
import phasetype_amd as P  # noqa: E402
import predict_ref as R  # noqa: E402
from phasetype_amd.synth import bd_exit_structure, simulate_ph  # noqa: E402

pytestmark = pytest.mark.gpu

ECS, UNIF = 2, 8
SCALES = (0.8, 1.0, 1.25)


def _gen(n):
    return R.one_state() if n == 1 else (R.ring(5) if n == 5 else R.bd(n))


def _scaled(S, s, scales=SCALES):
    return [c * S for c in scales], [c * s for c in scales]


def _sweeper(n, method=ECS):
    return P.Sweeper(n, method, 1, device=0)


@pytest.mark.parametrize("n", [1, 3, 5, 10, 32])
def test_pointwise_bit_exact(gpu, n):
    S, s = _gen(n)
    Ss, ss = _scaled(S, s)
    edges = np.linspace(0.1, 3.0, 16) * R.moments(S)[0]
    want = R.predict(Ss, ss, 1000, edges=edges)
    assert np.all(want["nbad"] == 0) and np.all(np.isfinite(want["y"]))
    sw = _sweeper(n)
    got = sw.predict(Ss, ss, 1000, key=R.KEY, edges=edges, pointwise=True)
    R.assert_same(got, want)
    totals = sw.predict(Ss, ss, 1000, key=R.KEY, edges=edges)  # the kernel without the pointwise stores
    sw.close()
    assert "y" not in totals
    R.assert_same(totals, want, pointwise=False)
    assert np.array_equal(R.bits(got["mean"]), R.bits(want["mean"])) and np.array_equal(got["ecdf"], want["ecdf"])


@pytest.fixture(scope="module")
def sweepers(gpu):
    """one context per n for the cases of evaluator_cases.OFF_BD_GPU"""
    held = {}

    def get(n):
        if n not in held:
            held[n] = _sweeper(n)
        return held[n]

    yield get
    for sw in held.values():
        sw.close()


def _paths_clean(r):
    """no draw flagged, no replicate bad, every value finite"""
    assert not np.asarray(r["flags"]).any() and not np.asarray(r["nbad"]).any() and np.all(r["ndone"] == 257)
    assert np.all(np.isfinite(r["y"])) and np.all(r["y"] > 0) and np.all(r["jumps"] >= 1)
    assert np.all(np.isfinite(r["ymin"])) and np.all(np.isfinite(r["ymax"])) and np.all(np.isfinite(r["mean"]))


@pytest.mark.parametrize("case", EC.OFF_BD_GPU, ids=EC.case_id)
def test_off_bd_exit_bit_equal_to_the_restatement(gpu, sweepers, case):
    """The families of tests/evaluator_cases.py through the jump selection:
    rows with a single successor (the chain families: every jump probability 0
    or 1 but for coxian_shared's exits), exit rates of exactly 0, holding rates
    over four decades (stiff).  5 draws, 257 replicates, 16 edges at
    0.1 .. 3 x the mean; batch 64 and 2."""
    family, n, kw = case
    S, s = EC.generator(family, n, **kw)
    Ss, ss = U.scaled(S, s)
    edges = np.linspace(0.1, 3.0, 16) * R.moments(S)[0]
    want = R.predict(Ss, ss, 257, edges=edges)
    _paths_clean(want)
    if family in ("erlang", "gapped", "hypoexp"):  # one way through the chain
        assert np.all(want["jumps"] == n)
    sw = sweepers(n)
    for batch in (64, 2):
        got = sw.predict(Ss, ss, 257, key=R.KEY, edges=edges, batch=batch, pointwise=True)
        _paths_clean(got)
        R.assert_same(got, want)
        assert np.array_equal(R.bits(got["mean"]), R.bits(want["mean"])) and np.array_equal(got["ecdf"], want["ecdf"])


@pytest.fixture(scope="module")
def shapes_want():
    """the restatement's 65 draws x 257 replicates of ring(5), computed once:
    fewer draws and replicates are its leading rows and columns"""
    S, s = R.ring(5)
    scales = 0.8 + 0.007 * np.arange(65)
    Ss, ss = _scaled(S, s, scales)
    return Ss, ss, R.predict(Ss, ss, 257)


@pytest.mark.parametrize("nd", [1, 2, 65])
def test_shapes_of_draws_batches_and_replicates(gpu, shapes_want, nd):
    Ss, ss, want = shapes_want
    sw = _sweeper(5)
    for nrep in (1, 63, 64, 65, 257):
        w = R.predict(Ss[:nd], ss[:nd], nrep)  # (the words of a shorter run are not a prefix: recomputed)
        assert np.array_equal(R.bits(w["y"]), R.bits(want["y"][:nd, :nrep]))
        for batch in (1, 2, 64):
            got = sw.predict(Ss[:nd], ss[:nd], nrep, key=R.KEY, batch=batch, pointwise=True)
            R.assert_same(got, w)
    sw.close()


@pytest.mark.parametrize("ne", [0, 1, 1024])
def test_edge_counts(gpu, ne):
    S, s = R.ring(5)
    Ss, ss = _scaled(S, s)
    edges = np.linspace(0.01, 12.0, ne) if ne > 1 else np.full(ne, 2.0)
    want = R.predict(Ss, ss, 3000, edges=edges)
    sw = _sweeper(5)
    got = sw.predict(Ss, ss, 3000, key=R.KEY, edges=edges, pointwise=True)
    sw.close()
    R.assert_same(got, want)
    assert got["counts"].shape == (3, ne + 1) and np.all(got["counts"].sum(axis=1) == 3000)
    for d in range(3):
        assert np.array_equal(got["counts"][d], np.bincount(np.searchsorted(edges, got["y"][d], "right"),
                                                            minlength=ne + 1))


def test_long_divergent_paths_and_a_mixed_batch(gpu):
    S, s = R.ring(5, exit_div=560.0)
    jm = R.jump_moments(S)[0]
    assert 1500 < jm < 2500, jm  # a path averages about 2000 jumps, some many times that
    want = R.predict([S], [s], 512)
    assert want["nbad"][0] == 0 and want["jumps"][0].max() > 4 * want["jumps"][0].min()
    sw = _sweeper(5)
    got = sw.predict([S], [s], 512, key=R.KEY, pointwise=True)
    R.assert_same(got, want)
    Sb, sb = R.bd(5)
    Ss, ss = [Sb, S, 1.1 * Sb, 0.9 * S], [sb, s, 1.1 * sb, 0.9 * s]
    edges = np.array([0.5, 5.0, 50.0, 500.0])
    for batch in (1, 4):
        R.assert_same(sw.predict(Ss, ss, 300, key=R.KEY, edges=edges, batch=batch, pointwise=True),
                      R.predict(Ss, ss, 300, edges=edges))
    sw.close()


def test_replicate_and_draw_splits_add(gpu):
    S, s = R.ring(5)
    Ss, ss = _scaled(S, s, (0.8, 0.9, 1.0, 1.1, 1.25))
    edges = np.linspace(0.2, 8.0, 16)
    sw = _sweeper(5)
    kw = dict(key=R.KEY, edges=edges, pointwise=True)
    whole = sw.predict(Ss, ss, 100, **kw)
    parts = P.predict_combine(sw.predict(Ss, ss, 37, rep0=0, **kw), sw.predict(Ss, ss, 63, rep0=37, **kw))
    R.assert_same(parts, whole)
    assert np.array_equal(R.bits(parts["mean"]), R.bits(whole["mean"]))
    R.assert_same(whole, R.predict(Ss, ss, 100, edges=edges))
    lo, hi = sw.predict(Ss[:2], ss[:2], 100, **kw), sw.predict(Ss[2:], ss[2:], 100, draw0=2, **kw)
    sw.close()
    for k in ("words", "counts", "ymin", "ymax", "y", "jumps"):
        assert np.array_equal(np.concatenate([lo[k], hi[k]]), whole[k]), k


def test_flagged_draw_horizon_and_cap(gpu):
    S, s = R.bd(3)
    bad = S.copy()
    bad[1, 1] = 0.0
    sw = _sweeper(3)
    for batch in (1, 64):
        got = sw.predict([S, bad, 1.1 * S], [s, s, 1.1 * s], 300, key=R.KEY, edges=[0.5, 1.0], batch=batch,
                         pointwise=True)
        assert list(got["flags"]) == [0, P.LL_F_MU, 0] and not got["words"][1].any() and np.all(np.isnan(got["y"][1]))
        R.assert_same(got, R.predict([S, bad, 1.1 * S], [s, s, 1.1 * s], 300, edges=[0.5, 1.0]))
    with pytest.raises(P.PhaseTypeError, match="edges"):
        sw.predict([S], [s], 10, edges=[1.0, 1.0])
    with pytest.raises(P.PhaseTypeError, match="max_jumps"):
        sw.predict([S], [s], 10, max_jumps=0)
    with pytest.raises(P.PhaseTypeError, match="horizon"):
        sw.predict([S], [s], 10, horizon=0.0)
    with pytest.raises(P.PhaseTypeError, match="2\\^32"):
        sw.predict([S], [s], 10, rep0=2 ** 32 - 5)
    sw.close()

    S, s = R.bd(10)
    hz = R.moments(S)[0]
    sw = _sweeper(10)
    got = sw.predict([S], [s], 5000, key=R.KEY, horizon=hz, edges=[0.5 * hz, hz], pointwise=True)
    free = sw.predict([S], [s], 5000, key=R.KEY, pointwise=True)
    sw.close()
    R.assert_same(got, R.predict([S], [s], 5000, horizon=hz, edges=[0.5 * hz, hz]))
    y = got["y"][0]
    assert got["nsurv"][0] == np.sum(y == hz) > 0 and np.all(y <= hz)
    assert np.array_equal(R.bits(y[y < hz]), R.bits(free["y"][0][y < hz]))

    S, s = R.ring(5, exit_div=1e3)
    sw = _sweeper(5)
    got = sw.predict([S], [s], 2000, key=R.KEY, max_jumps=64, edges=[1.0, 10.0], pointwise=True)
    sw.close()
    R.assert_same(got, R.predict([S], [s], 2000, max_jumps=64, edges=[1.0, 10.0]))
    assert got["nbad"][0] > 0 and got["ndone"][0] + got["nbad"][0] == 2000
    bad = np.isnan(got["y"][0])
    assert bad.sum() == got["nbad"][0] and np.all(got["jumps"][0][bad] == 64)


def _cyclic_structure():
    """T of the 3-cycle 1 -> 2 -> 3 -> 1 with an exit from every state"""
    T = np.zeros((4, 4), np.int32)
    T[0, 1], T[0, 3], T[1, 2], T[1, 3], T[2, 0], T[2, 3] = 1, 2, 3, 4, 5, 6
    return T, np.array([1.0, 0.1, 1.0, 0.1, 1.0, 0.1])


@pytest.mark.parametrize("method", [ECS, UNIF])
def test_the_chain_and_the_loglik_are_untouched(gpu, method):
    n, it = 3, 6
    T, theta = bd_exit_structure(3) if method == ECS else _cyclic_structure()
    S, s = P.theta_to_S(theta, T)
    y, cen = simulate_ph(S, s, 1000, seed=15, censor_frac=0.3)
    nu, zeta, Cm, zexp = 1 + 50 * theta, np.full(len(theta), 50.0), np.ones(T.shape), P.zexp_for(y)

    def chain(with_predict):
        P.set_seed(1)
        sw = P.Sweeper(n, method, 1, device=0)
        if with_predict:  # a context with no observations set
            r = sw.predict([S, 1.1 * S], [s, 1.1 * s], 500, key=R.KEY, edges=[0.5, 2.0])
            assert np.all(r["ndone"] == 500)
        sw.set_obs(y, cen)
        ll0 = sw.loglik_unif([S], [s], pointwise=True)
        a = sw.gibbs(it, method, nu, zeta, T, Cm, zexp)
        if with_predict:
            sw.predict([S], [s], 2000, key=(3, 4), pointwise=True)
        b = sw.gibbs(it, method, nu, zeta, T, Cm, zexp, start=a[-1])
        ll1 = sw.loglik_unif([S], [s], pointwise=True)
        sw.close()
        assert np.array_equal(R.bits(ll0["pointwise"]), R.bits(ll1["pointwise"])) and ll0["total"][0] == ll1["total"][0]
        return np.concatenate([a, b]), ll1["pointwise"]

    with_c, with_l = chain(True)
    without_c, without_l = chain(False)
    assert np.array_equal(R.bits(with_c), R.bits(without_c))
    assert np.array_equal(R.bits(with_l), R.bits(without_l))


def test_end_to_end_ppc_and_rph(gpu):
    S, s = R.bd(3)
    x, _ = simulate_ph(S, s, 2000, seed=21)
    TT = np.array([["0", "f1", "0", "e1"], ["b1", "0", "f2", "e2"], ["0", "b2", "0", "e3"], ["0", "0", "0", "0"]],
                  dtype=object)
    truth = dict(f1=2.0, f2=2.0, b1=0.5, b2=0.5, e1=0.3, e2=0.3, e3=2.0)
    P.set_seed(7)
    res = P.phtMCMC2(x, TT, [1, 0, 0], {k: 1 + 50 * v for k, v in truth.items()}, {k: 50.0 for k in truth}, 60,
                     silent=True)
    out = P.ppc(res, x, burn=10)
    assert out["n_draws_used"] == 50 and out["predict"]["ndone"].min() == 2000
    for name, p in out["p"].items():
        assert np.isfinite(p) and 0.0 <= p <= 1.0, (name, p)
    k = int(np.searchsorted(out["edges"], np.median(x)))
    assert out["band"][0][k] <= out["ecdf_x"][k] <= out["band"][2][k], (out["band"][:, k], out["ecdf_x"][k])
    # administrative censoring: data and replicates recorded at the horizon
    hz = float(np.quantile(x, 0.9))
    xc, cen = np.minimum(x, hz), (x >= hz).astype(np.int32)
    outc = P.ppc(res, xc, censored=cen, horizon=hz, burn=10, nrep=1000)
    assert outc["predict"]["nsurv"].min() > 0 and outc["T_x"]["max"] == hz
    assert all(0.0 <= p <= 1.0 for p in outc["p"].values())

    N = 100000
    y = P.rph(S, s, N, key=R.KEY)
    assert y.shape == (N,) and np.all(np.isfinite(y))
    ys = np.sort(y)
    grid = np.linspace(0.05, 4.0, 64) * R.moments(S)[0]
    D = float(np.max(np.abs(np.searchsorted(ys, grid, "right") / N - R.cdf(S, grid))))
    print(f"rph: sup|ecdf - F| {D:.6f}, DKW bound {R.dkw(N):.6f}")
    assert D <= R.dkw(N)
    assert np.array_equal(R.bits(y[:1000]), R.bits(R.predict([S], [s], 1000)["y"][0]))  # variate i = replicate i
