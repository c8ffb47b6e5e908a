"""GPU: the uniformisation analyses share one staging path and one input and
table buffer on the context (phasetype_amd/csrc/host_unif.cpp): on a single
Sweeper, calls of every analysis in turn, with a growing then shrinking number
of draws, tables of mixed length and a flagged draw mid-batch, each give bit
for bit what the restatements (tests/*_ref.py) give for that call alone, and
each call's device times land in its own analysis' clock and in no other."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import condition_ref as Cd  # noqa: E402
import estep_ref as E  # noqa: E402
import forecast_ref as F  # noqa: E402
import loglik_ref as R  # noqa: E402
import loglik_unif_ref as U  # noqa: E402
import phasetype_amd as P  # noqa: E402
import psis_ref as Ps  # noqa: E402
import quantile_ref as Q  # noqa: E402
from phasetype_amd.synth import bd_exit  # noqa: E402

pytestmark = pytest.mark.gpu

ECS = 2
N, NCENS, ND, NAN_AT = 48, 16, 7, 3
CLOCKS = ("estep", "quantile", "forecast", "condition")
H2 = np.array([0.5, 2.0])
PROBS = np.array([0.5, 0.05, 0.95, 0.25, 0.75])


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _case():
    """7 draws of BD-exit(3), every other one 40 times as fast (its table is
    many times as long), draw 3 with a NaN; 48 observations, 16 censored"""
    S, s = bd_exit(3)
    scales = [(40.0 if d & 1 else 1.0) * (1.0 + 0.01 * d) for d in range(ND)]
    Ss, ss = [S * c for c in scales], [s * c for c in scales]
    Ss[NAN_AT][1, 0] = np.nan
    rng = np.random.default_rng(16)
    y = np.round(rng.exponential(1.5, N), 2) + 0.01
    cens = np.zeros(N, np.int32)
    cens[rng.permutation(N)[:NCENS]] = 1
    return Ss, ss, y, cens


def _clocks(sw):
    """the four analyses' device-time pairs, read from the context"""
    out = {}
    for k in CLOCKS:
        a, b = C.c_float(0), C.c_float(0)
        assert getattr(sw.L, f"pht_ctx_{k}_ms")(sw.ctx, C.byref(a), C.byref(b)) == 0
        out[k] = (a.value, b.value)
    return out


def _timed(sw, before, which):
    """after a call: ``which``'s pair is the call's (None: no analysis with a
    clock ran), every other pair is as before; returns the pairs now"""
    now = _clocks(sw)
    for k in CLOCKS:
        if k == which:
            assert all(np.isfinite(v) and v >= 0.0 for v in now[k]), (k, now[k])
            assert getattr(sw, f"last_{k}_ms") == now[k]
        else:
            assert now[k] == before[k], (which, k, before[k], now[k])
    return now


def _loglik_same(got, want_pw, bad):
    assert np.array_equal(_bits(got["pointwise"]), _bits(want_pw))
    words = R.totals(want_pw)
    words[bad] = 0
    assert np.array_equal(np.stack([got[k] for k in ("H", "F", "nbad", "nobs")], axis=1), words)
    assert np.array_equal(got["bad_draw"], bad)


def test_every_analysis_in_turn_on_one_context(gpu):
    Ss, ss, y, cens = _case()
    bad = np.arange(ND) == NAN_AT
    sw = P.Sweeper(3, ECS, 1, device=0)
    try:
        sw.set_obs(y, cens)
        # tables of mixed length, none at the cap
        Ks = [sw.loglik_unif_K(np.max(-np.diag(Ss[d]))) for d in (0, 1)]
        assert Ks[0] * 4 < Ks[1] < 2047, Ks
        clk = _clocks(sw)

        got = sw.loglik_unif(Ss[:5], ss[:5], batch=2, pointwise=True)
        _loglik_same(got, U.pointwise(Ss[:5], ss[:5], y, cens), bad[:5])
        clk = _timed(sw, clk, None)

        got = sw.condition(Ss[:2], ss[:2], H2, batch=2, pointwise=True)
        want = Cd.condition(Ss[:2], ss[:2], y, cens, H2)
        assert Cd.same_bits(got, want, Cd.KEYS + Cd.POINT + Cd.DERIVED) == []
        clk = _timed(sw, clk, "condition")

        got = sw.estep(Ss, ss, batch=2)
        for d in range(ND):
            w = E.estep(Ss[d], ss[d], y, cens)
            assert int(got["flags"][d]) == w["flag"] and (w["flag"] != 0) == bad[d], d
            assert np.array_equal(got["words"][d], w["words"]), d
            assert [int(got[k][d]) for k in ("H", "F", "nbad", "nobs")] == [int(v) for v in w["totals"]], d
            for k in ("Z", "N", "E", "A", "loglik"):
                assert np.array_equal(_bits(got[k][d]), _bits(w[k])), (d, k)
        clk = _timed(sw, clk, "estep")

        got = sw.quantile(Ss[:3], ss[:3], PROBS, batch=2)
        want = Q.quantile(Ss[:3], ss[:3], PROBS)
        for k in ("t", "lo", "hi"):
            assert np.array_equal(_bits(got[k]), _bits(want[k])), k
        for k in ("nev", "flags", "bad_draw", "draw_flags"):
            assert np.array_equal(got[k], want[k]), k
        clk = _timed(sw, clk, "quantile")

        got = sw.forecast(Ss, ss, H2, batch=2, pointwise=True)
        want = F.forecast(Ss, ss, y, cens, H2)
        assert F.same_bits(got, want, F.KEYS + ("q", "M", "V", "nbad", "nunits", "p_unit")) == []
        assert np.array_equal(got["bad_draw"], bad)
        clk = _timed(sw, clk, "forecast")

        sw.loo_begin(5)
        tot, bad_rows = sw.loo_fill(0, Ss[:5], ss[:5], batch=2, unif=True)
        got = sw.loo_result()
        sw.loo_end()
        pw = U.pointwise(Ss[:5], ss[:5], y, cens)
        words = R.totals(pw)
        words[bad[:5]] = 0
        assert np.array_equal(tot, words) and np.array_equal(bad_rows, bad[:5])
        want = Ps.psis(pw, ~bad[:5])
        for k in ("elpd_i", "khat", "lppd_i"):
            assert np.array_equal(_bits(got[k]), _bits(want[k])), k
        assert np.array_equal(got["flags"], want["flags"]) and got["n_draws_used"] == 4
        clk = _timed(sw, clk, None)

        got = sw.loglik_unif(Ss[:1], ss[:1], batch=2, pointwise=True)
        _loglik_same(got, U.pointwise(Ss[:1], ss[:1], y, cens), bad[:1])
        _timed(sw, clk, None)
    finally:
        sw.close()
