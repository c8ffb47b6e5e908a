"""GPU: the quantile kernel (phasetype_amd/csrc/pht_quantile.hip) against the
tests' restatement of include/pht_quantile.h (tests/quantile_spec.c), bit for
bit in every output word; consistency with the log-likelihood evaluator and
with rph; no interference with the WAIC state, the totals and a chain;
ph_quantiles and qph end to end."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import evaluator_cases as EC  # noqa: E402
import loglik_unif_ref as U  # noqa: E402
import quantile_ref as Q  # noqa: E402
import phasetype_amd as P  # noqa: E402
from phasetype_amd.synth import bd_exit, simulate_ph  # noqa: E402

pytestmark = pytest.mark.gpu

ECS, UNIF = 2, 8
EDGES = [0.0, 1.0, np.nan, -0.1, 1e-6, 1 - 1e-9, 0.5, 0.5]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _gen(n):
    return {1: (np.array([[-0.7]]), np.array([0.7])), 3: U.CYCLIC, 5: U.ring(5)}.get(n) or bd_exit(n)


def _probs(P_, seed=3):
    """P_ probabilities in no order: ordinary ones with, from eight on, the
    edge values, a NaN, one outside [0, 1] and a duplicate among them"""
    rng = np.random.default_rng(seed)
    if P_ < len(EDGES):
        return rng.uniform(0.01, 0.99, P_)
    p = np.concatenate([rng.uniform(0.001, 0.999, P_ - len(EDGES)), EDGES])
    return p[rng.permutation(P_)]


def _draws(n, nd, tmax):
    """nd draws (the generator scaled by 0.8 .. 1.25).  With three or more:
    draw 1 carries a NaN, draw 2 has its exit rates cut to 1e-6 of theirs (its
    roots lie beyond the horizon), and with exactly three and a finite tmax
    draw 0 is so fast that mu tmax exceeds 1400: its table reaches the cap."""
    S, s = _gen(n)
    scales = np.linspace(0.8, 1.25, nd) if nd > 1 else np.array([1.0])
    Ss, ss = [S * c for c in scales], [s * c for c in scales]
    if nd >= 3:
        Ss[1] = Ss[1].copy()
        Ss[1][0, 0] = np.nan
        Ss[2], ss[2] = Ss[2] + np.diag(ss[2]) - np.diag(ss[2] * 1e-6), ss[2] * 1e-6
        if nd == 3 and tmax is not None:
            c = 2000.0 / (np.max(-np.diag(S)) * tmax)
            Ss[0], ss[0] = S * c, s * c
    return Ss, ss


def _check(got, want, tag):
    for k in ("t", "lo", "hi"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (tag, k)
    for k in ("nev", "flags", "bad_draw", "draw_flags"):
        assert np.array_equal(got[k], want[k]), (tag, k)


# n x draws (1 / 3 / 65: across the batch of 64) x P (1, 63, 64, 65, 300: wave
# and block edges, several draws a block) x batch (1 / 7 / 64) x given x tmax
CASES = [(1, 1, 1, 64, 0.0, None), (1, 3, 63, 1, 0.5, 4.0), (1, 65, 300, 7, 0.0, None),
         (3, 3, 64, 7, 0.0, None), (3, 65, 65, 64, 2.0, None), (3, 1, 300, 64, 0.0, 50.0),
         (5, 3, 300, 64, 0.0, None), (5, 65, 1, 64, 1.0, 40.0),
         (10, 65, 63, 7, 0.0, 30.0), (10, 3, 65, 1, 1.5, None), (10, 1, 300, 64, 0.0, None), (10, 65, 1, 64, 0.0, 30.0),
         (10, 3, 64, 64, 0.5, 30.0), (32, 3, 64, 64, 0.0, None), (32, 65, 1, 64, 1.0, None), (32, 1, 63, 1, 0.0, 20.0),
         (32, 3, 300, 7, 2.0, 25.0)]


@pytest.mark.parametrize("n,nd,P_,batch,given,tmax", CASES)
def test_bit_equal_to_the_restatement(gpu, n, nd, P_, batch, given, tmax):
    Ss, ss = _draws(n, nd, tmax)
    probs = _probs(P_)
    want = Q.quantile(Ss, ss, probs, given=given, tmax=np.inf if tmax is None else tmax)
    if nd >= 3:
        assert want["bad_draw"][1] and np.all(want["flags"][1] == Q.F_DRAW)
        if n > 1:
            assert (want["flags"][2] & Q.F_BEYOND).any()
        if nd == 3 and tmax is not None:
            assert Q.meta(Ss[0], ss[0], tmax)["K"] == 1988  # the cap's table
    assert not (want["flags"] & Q.F_CAP).any()
    sw = P.Sweeper(n, ECS, 1, device=0)
    got = sw.quantile(Ss, ss, probs, given=given, tmax=tmax, batch=batch)
    sw.close()
    _check(got, want, (n, nd, P_, batch, given, tmax))


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


def _roots_clean(r, family):
    """no draw flagged, every root found and finite.  On ``stiff`` the slowest
    phases put the upper quantiles beyond the table's horizon, as
    tests/test_quantile.py documents: PHT_Q_F_BEYOND and no other flag, and at
    least 10 of the 30 roots finite"""
    assert not r["bad_draw"].any() and not r["draw_flags"].any()
    assert r["t"].shape == (5, len(EC.QUANTILE_P)) and np.all(r["nev"] >= 1)
    if family == "stiff":
        assert set(np.unique(r["flags"]).tolist()) <= {0, Q.F_BEYOND}
        assert np.isfinite(r["t"]).sum() >= 10
    else:
        assert not r["flags"].any() and np.all(np.isfinite(r["t"]))
    ok = r["flags"] == 0
    assert np.all(np.isfinite(r["t"][ok])) and np.all(r["t"][ok] > 0) and np.all(np.isinf(r["t"][~ok]))
    assert np.all(np.isfinite(r["lo"][ok])) and np.all(np.isfinite(r["hi"][ok]))


@pytest.mark.parametrize("case", EC.OFF_BD_GPU, ids=EC.case_id)
def test_off_bd_exit_bit_equal_to_the_restatement(gpu, sweepers, case):
    """The families of tests/evaluator_cases.py through the bracketed Newton
    lanes: f(t) ~ t^(n - 1) at the lower quantiles of the chain families (up
    to 98 evaluations a root on Erlang(3)), a shift for R, rates over four
    decades.
    5 draws, the probabilities 1e-6 .. 1 - 1e-9, unconditional and given
    survival to the fleet's second-largest age; batch 64 and 2."""
    S, s, y, cens, _ = EC.off_bd_case(case)
    n = S.shape[0]
    Ss, ss = U.scaled(S, s)
    probs = np.array(EC.QUANTILE_P)
    given = float(np.unique(y[cens != 0])[-2])
    sw = sweepers(n)
    for g in (0.0, given):
        want = Q.quantile(Ss, ss, probs, given=g)
        _roots_clean(want, case[0])
        assert want["nev"].max() < Q.spec().qspec_maxit()
        for batch in (64, 2):
            got = sw.quantile(Ss, ss, probs, given=g, batch=batch)
            _roots_clean(got, case[0])
            _check(got, want, (EC.case_id(case), g, batch))


@pytest.fixture(scope="module")
def case10(gpu):
    Ss, ss = _draws(10, 5, None)
    probs = np.array([0.9, 1e-3, 0.5, 0.1, 1 - 1e-9, 1e-6])
    sw = P.Sweeper(10, ECS, 1, device=0)
    out = {g: sw.quantile(Ss, ss, probs, given=g) for g in (0.0, 1.5)}
    sw.close()
    return Ss, ss, probs, out


def test_consistent_with_the_loglik_evaluator(gpu, case10):
    """the roots as censored observations: Sweeper.loglik_unif's pointwise
    log survival is log(1 - p) + lS(t0) within the header's bound plus that
    evaluation's own"""
    Ss, ss, probs, out = case10
    for given, r in out.items():
        for d in (0, 3, 4):
            S, s = Ss[d], ss[d]
            t = r["t"][d] + given
            assert np.all(np.isfinite(t)) and not r["flags"][d].any()
            obs = np.concatenate([t, [given]]) if given > 0 else t
            sw = P.Sweeper(10, ECS, 1, device=0)
            sw.set_obs(obs, np.ones(len(obs), np.int32))
            pw = sw.loglik_unif([S], [s], pointwise=True)["pointwise"][0]
            sw.close()
            _, khi = U.pointwise([S], [s], obs, np.ones(len(obs), np.int32), with_khi=True)
            eps = U.bound(10, khi[0])
            l0, e0 = (pw[-1], eps[-1]) if given > 0 else (0.0, 0.0)
            tol = Q.bound(S, s, probs, r["lo"][d], r["hi"][d], given=given) + eps[:len(t)] + e0
            tol = tol + ss[d].max() * 2.0 ** -52 * t  # t^ + t0 rounds once more
            err = np.abs(pw[:len(t)] - (np.log1p(-probs) + l0))
            print(f"given {given} draw {d}: largest error / tolerance {np.max(err / tol):.3f}")
            assert np.all(err <= tol), (given, d, err, tol)


def test_against_rph(gpu):
    """2^20 replicates of one bd_exit(4) draw under a fixed key: the count at
    or below the quantile lies within 5 sqrt(N p (1 - p)) of N p"""
    S, s = bd_exit(4)
    N = 1 << 20
    p = np.array([0.1, 0.5, 0.9])
    q = P.qph(S, s, p)
    y = P.rph(S, s, N, key=(11, 12))
    assert np.all(np.isfinite(y)) and np.all(np.diff(q) > 0)
    cnt = np.array([(y <= v).sum() for v in q])
    print("counts - N p over sqrt(N p (1 - p)):", (cnt - N * p) / np.sqrt(N * p * (1 - p)))
    assert np.all(np.abs(cnt - N * p) <= 5 * np.sqrt(N * p * (1 - p)))
    assert isinstance(P.qph(S, s, 0.5), float) and P.qph(S, s, 0.5) == q[1]
    # the family agrees with itself: pph(qph(p)) = p, dph = the hazard's density
    # (an evaluation's bound at the table cap, and the root's own)
    r = Q.quantile([S], [s], p)
    eps, b = float(U.bound(4, 1988)), Q.bound(S, s, p, r["lo"][0], r["hi"][0])
    assert np.all(np.abs(P.pph(S, s, q) - p) <= (eps + b) * (1 - p) * 1.000001)
    assert np.all(np.abs(np.log(P.dph(S, s, q)) - np.log(Q.hazard(S, s, q) * (1 - p))) <= 3 * eps + b)


def test_waic_totals_and_chain_are_untouched(gpu):
    n, it = 3, 6
    T = np.zeros((4, 4), np.int32)
    T[0, 1], T[0, 3], T[1, 2], T[1, 3], T[2, 0], T[2, 3] = 1, 2, 3, 4, 5, 6
    theta = np.array([1.0, 0.1, 1.0, 0.1, 1.0, 0.1])
    S, s = P.theta_to_S(theta, T)
    y, cen = simulate_ph(S, s, 1000, seed=15, censor_frac=0.3)
    nu, zeta, Cm, zexp = 1 + 50 * theta, np.full(len(theta), 50.0), np.ones(T.shape), P.zexp_for(y)
    pr = np.array([0.3, 0.999, 0.0, 0.5])

    def run(with_q):
        P.set_seed(1)
        sw = P.Sweeper(n, UNIF, 1, device=0)
        sw.set_obs(y, cen)
        sw.waic_reset()
        if with_q:
            sw.quantile([S, 1.1 * S], [s, 1.1 * s], pr)
        a = sw.loglik_unif([S, 1.1 * S], [s, 1.1 * s], accumulate=True)
        if with_q:
            sw.quantile([S], [s], pr, given=2.0, batch=1)
        c1 = sw.gibbs(it, UNIF, nu, zeta, T, Cm, zexp)
        if with_q:
            sw.quantile([0.9 * S] * 65, [0.9 * s] * 65, pr, tmax=5.0)
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
        assert np.array_equal(_bits(wst[k]), _bits(st[k])), k
    assert np.array_equal(wst["cnt"], st["cnt"])
    assert np.array_equal(_bits(wc), _bits(c))


def test_end_to_end_ph_quantiles_and_qph(gpu):
    S, s = bd_exit(3)
    x, _ = simulate_ph(S, s, 500, seed=21)
    TT = np.array([["0", "f1", "0", "e1"], ["b1", "0", "f2", "e2"], ["0", "b2", "0", "e3"], ["0", "0", "0", "0"]],
                  dtype=object)
    truth = dict(f1=2.0, f2=2.0, b1=0.5, b2=0.5, e1=0.3, e2=0.3, e3=2.0)
    P.set_seed(7)
    res = P.phtMCMC2(x, TT, [1, 0, 0], {k: 1 + 50 * v for k, v in truth.items()}, {k: 50.0 for k in truth}, 200,
                     silent=True)
    probs = [0.1, 0.5, 0.9]
    out = P.ph_quantiles(res, TT, probs, burn=20)
    assert out["q"].shape == (180, 3) and np.all(out["n_finite"] == 180)
    assert not out["n_beyond"].any() and not out["n_flagged"].any()
    assert np.all(np.isfinite(out["band"])) and np.all(np.diff(out["band"], axis=0) >= 0)
    assert np.all(np.diff(out["band"], axis=1) > 0)  # and increasing in p
    T, names = P._tt_numbers(TT)
    Sm, sm = P.theta_to_S(np.asarray(res["samples"], np.float64)[20:].mean(0), T)
    qm = P.qph(Sm, sm, np.array(probs))
    assert np.all(qm >= out["q"].min(0)) and np.all(qm <= out["q"].max(0))
    # the remaining life of a unit that has survived to the median
    rl = P.ph_quantiles(res, TT, probs, given=float(out["band"][1, 1]), burn=20, thin=4)
    assert rl["q"].shape == (45, 3) and np.all(np.isfinite(rl["band"])) and np.all(rl["q"] > 0)
    # a horizon below the roots: counted, not dropped
    short = P.ph_quantiles(res, TT, probs, burn=20, tmax=float(out["q"][:, 0].min()) / 2)
    assert np.all(short["n_beyond"] == 180) and np.all(short["n_finite"] == 0) and np.all(np.isnan(short["band"]))
