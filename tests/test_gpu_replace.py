"""GPU: the replacement kernels (phasetype_amd/csrc/pht_replace.hip) against
the tests' restatement of include/pht_replace.h (tests/replace_spec.c), bit for
bit in every output word: the curve (lS, lf, M, age flags), the policies (t, g,
lo, hi, j, nev, flags), m and the draws' flags; no interference with the
quantile and the spares calls on the same context; the one-draw wrappers."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import loglik_unif_ref as U  # noqa: E402
import quantile_ref as Q  # noqa: E402
import replace_ref as R  # noqa: E402
import spares_ref as Sp  # noqa: E402
import phasetype_amd as P  # noqa: E402
from phasetype_amd.synth import bd_exit  # noqa: E402

pytestmark = pytest.mark.gpu

ECS = 2
CP2, CF2 = [p[0] for p in R.PAIRS], [p[1] for p in R.PAIRS]
# 16 pairs: the two of the tests, ratios cf / cp from 1.05 to 1000, and three unusable ones
CP16 = np.array([1.0, 1.0, 1.0, 2.0, 1.0, 0.5, 1.0, 3.0, 1.0, 1.0, 1.0, 1e-3, 1.0, 0.0, 2.0, 1.0])
CF16 = np.array([10.0, 1.5, 1.05, 4.0, 3.0, 50.0, 100.0, 3.5, 1000.0, 2.0, 20.0, 1.0, 6.0, 1.0, 1.0, np.nan])


def _draws(S, s):
    """the five scalings of loglik_unif_ref.SCALES, then a draw with a NaN and a
    trapped one (state 1 never leaves: PHT_CD_F_TRAP)"""
    Ss, ss = U.scaled(S, s)
    Sn = S.copy()
    Sn[0, 0] = np.nan
    St, st = S.copy(), s.copy()
    if S.shape[0] > 1:
        St[0, 1:] = 0.0
        st[0] = 0.0
    else:
        st[0] = 0.0
    return Ss + [Sn, St], ss + [s, st]


def _ages(S, s, G):
    m = R.mean(S, s)
    return m * {1: np.array([0.4]), 7: R.GRID, 300: np.geomspace(0.02, 4.0, 300)}[G]


def _run(n, Ss, ss, ages, cp, cf, batch):
    sw = P.Sweeper(n, ECS, 1, device=0)
    try:
        return sw.replace(Ss, ss, ages, cp, cf, batch=batch, pointwise=True)
    finally:
        sw.close()


# (generator, G, pairs, batch): n = 3, 6, 10, 12; G = 1, 7 and 300 (across a tile
# of 256 lanes); P = 1, 2 and 16 (four blocks of four waves a draw); batch 64 and 2
CASES = [("bd3", 7, 2, 64), ("erlang6", 7, 2, 2), ("bd10", 300, 16, 64), ("neareq12", 1, 1, 64),
         ("hypoexp6", 300, 2, 3), ("reversible6", 7, 16, 64)]


@pytest.mark.parametrize("name,G,P_,batch", CASES)
def test_bit_equal_to_the_restatement(gpu, name, G, P_, batch):
    S, s = R.named(name)
    Ss, ss = _draws(S, s)
    ages = _ages(S, s, G)
    cp, cf = {1: ([1.0], [10.0]), 2: (CP2, CF2), 16: (CP16, CF16)}[P_]
    want = R.replace(Ss, ss, ages, cp, cf)
    assert want["draw_flags"][5] != 0 and want["draw_flags"][6] == R.F_TRAP
    assert np.all(want["flags"][5:] == R.F_DRAW) and np.all(want["age_flags"][5:] == R.A_DRAW)
    assert not want["draw_flags"][:5].any() and not (want["flags"] & R.F_CAP).any()
    if P_ == 16:
        bad_pair = ~((CP16 > 0) & (CF16 > CP16) & (CF16 < np.inf))
        assert bad_pair.sum() == 3 and np.all((want["flags"][:5] == R.F_COST) == bad_pair[None, :])
    got = _run(S.shape[0], Ss, ss, ages, cp, cf, batch)
    assert R.same_bits(got, want) == [], (name, G, P_, batch, R.same_bits(got, want))
    print(name, "flags", np.unique(got["flags"]), "largest nev", got["nev"].max())


def test_runtime_n_32_one_draw(gpu):
    S, s = bd_exit(32)
    ages = _ages(S, s, 7)
    want = R.replace([S], [s], ages, CP2, CF2)
    assert not want["bad_draw"].any() and not want["age_flags"].any()
    got = _run(32, [S], [s], ages, CP2, CF2, 64)
    assert R.same_bits(got, want) == []


def test_70_draws_cross_a_batch(gpu):
    S, s = R.named("bd3")
    scales = np.linspace(0.7, 1.4, 70)
    Ss, ss = [S * c for c in scales], [s * c for c in scales]
    Ss[66] = Ss[66].copy()
    Ss[66][1, 1] = np.inf
    ages = _ages(S, s, 7)
    want = R.replace(Ss, ss, ages, [1.0], [10.0])
    assert want["bad_draw"].sum() == 1 and (want["flags"] == 0).sum() >= 60
    got = _run(3, Ss, ss, ages, [1.0], [10.0], 64)
    assert R.same_bits(got, want) == []


def test_an_age_beyond_one_draws_horizon_and_an_unusable_pair(gpu):
    """draw 1 is so fast that the last two ages lie beyond mu tau = 1400: they
    are bad for that draw only, flagged, NaN, and its policy comes from the
    five good ages; the pair (2, 1) beside (1, 10) is PHT_RP_F_COST"""
    S, s = R.named("erlang6")
    ages = _ages(S, s, 7)
    mu = float(np.max(-np.diag(S)))
    c = 1400.0 / (mu * ages[4]) * 0.999
    Ss, ss = [S, S * c, 0.9 * S], [s, s * c, 0.9 * s]
    cp, cf = [1.0, 2.0], [10.0, 1.0]
    want = R.replace(Ss, ss, ages, cp, cf)
    assert not want["bad_draw"].any()
    assert np.all(want["age_flags"][1, 5:] == R.A_BEYOND) and not (want["age_flags"][1, :5] & R.A_BEYOND).any()
    assert (want["age_flags"][1] == 0).sum() >= 2
    assert not want["age_flags"][0].any() and not want["age_flags"][2].any()
    assert np.all(np.isnan(want["M"][1, 5:])) and np.all(np.isfinite(want["M"][1, want["age_flags"][1] == 0]))
    assert np.all(want["flags"][:, 1] == R.F_COST) and np.all(np.isnan(want["t"][:, 1]))
    assert want["flags"][0, 0] == 0 and not (want["flags"][1, 0] & (R.F_DRAW | R.F_NOAGE))
    got = _run(6, Ss, ss, ages, cp, cf, 64)
    assert R.same_bits(got, want) == []


def _clocks(sw):
    out = {}
    for k in ("quantile", "spares", "replace"):
        a, b = C.c_float(0), C.c_float(0)
        assert getattr(sw.L, f"pht_ctx_{k}_ms")(sw.ctx, C.byref(a), C.byref(b)) == 0
        out[k] = (a.value, b.value)
    return out


def test_between_quantile_and_spares_on_one_context(gpu):
    """replace between quantile and spares on one context leaves their results
    bit for bit a fresh context's, and moves only its own clock"""
    S, s = bd_exit(3)
    Ss, ss = U.scaled(S, s)
    Ss[2] = Ss[2].copy()
    Ss[2][1, 0] = np.nan
    rng = np.random.default_rng(5)
    y = np.round(rng.exponential(1.5, 40), 2) + 0.01
    cens = (np.arange(40) % 3 == 0).astype(np.int32)
    probs, H = np.array([0.5, 0.05, 0.95]), np.array([0.5, 2.0])
    ages = _ages(S, s, 7)

    def fresh():
        sw = P.Sweeper(3, ECS, 1, device=0)
        sw.set_obs(y, cens)
        return sw

    sw = fresh()
    try:
        q1 = sw.quantile(Ss, ss, probs, batch=2)
        c1 = _clocks(sw)
        r = sw.replace(Ss, ss, ages, CP2, CF2, batch=2, pointwise=True)
        c2 = _clocks(sw)
        assert c2["quantile"] == c1["quantile"] and c2["spares"] == c1["spares"]
        assert sw.last_replace_ms == c2["replace"] and all(np.isfinite(v) and v >= 0 for v in c2["replace"])
        assert c2["replace"][0] > 0 and c2["replace"][1] > 0
        s1 = sw.spares(Ss, ss, H, batch=2, pointwise=True)
        c3 = _clocks(sw)
        assert c3["quantile"] == c2["quantile"] and c3["replace"] == c2["replace"]
        q2 = sw.quantile(Ss, ss, probs, batch=2)
    finally:
        sw.close()
    assert R.same_bits(r, R.replace(Ss, ss, ages, CP2, CF2)) == []
    a, b = fresh(), fresh()
    try:
        q0 = a.quantile(Ss, ss, probs, batch=2)
        s0 = b.spares(Ss, ss, H, batch=2, pointwise=True)
    finally:
        a.close()
        b.close()
    for q in (q1, q2):
        for k in ("t", "lo", "hi"):
            assert np.array_equal(q[k].view(np.uint64), q0[k].view(np.uint64)), k
        for k in ("nev", "flags", "bad_draw", "draw_flags"):
            assert np.array_equal(q[k], q0[k]), k
    want = Q.quantile(Ss, ss, probs)
    assert np.array_equal(q0["t"].view(np.uint64), want["t"].view(np.uint64))
    assert set(s1) == set(s0)
    for k, v in s0.items():
        if isinstance(v, np.ndarray):
            assert v.dtype == s1[k].dtype and v.tobytes() == s1[k].tobytes(), k
    assert Sp.same_bits(s1, Sp.spares(Ss, ss, y, cens, H), Sp.KEYS) == []


def test_one_draw_wrappers(gpu):
    S, s = R.named("erlang6")
    m = R.mean(S, s)
    r = P.age_replacement(S, s, 1.0, 10.0, ages=m * R.GRID)
    want = R.replace([S], [s], m * R.GRID, [1.0], [10.0])
    assert r["flags"][0] == 0 and r["t"][0] == want["t"][0, 0] and r["g"][0] == want["g"][0, 0] and r["m"] == m
    d = P.age_replacement(S, s, 1.0, 10.0)  # the default grid: 64 ages over 0.02 .. 8 mean lives
    assert d["flags"][0] == 0 and len(d["ages"]) == 64 and abs(d["t"][0] / want["t"][0, 0] - 1) < 1e-9
    tau = np.array([[0.0, m], [2 * m, 0.5 * m]])
    M = P.ph_rmean(S, s, tau)
    assert M.shape == (2, 2) and M[0, 0] == 0.0
    ref = R.rmean(S, s, np.array([0.5 * m, m, 2 * m]))["M"]
    assert np.array_equal(M.reshape(-1)[[3, 1, 2]], ref)
    assert isinstance(P.ph_rmean(S, s, m), float) and P.ph_rmean(S, s, m) == ref[1]
    with pytest.raises(P.PhaseTypeError, match="strictly increasing"):
        _run(6, [S], [s], [1.0, 1.0], [1.0], [2.0], 64)
    with pytest.raises(P.PhaseTypeError, match="cost pairs"):
        _run(6, [S], [s], [1.0], np.ones(17), 2 * np.ones(17), 64)
