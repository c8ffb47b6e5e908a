"""The converged ECS round after its instruction-count work (fewer position
tests in meets / cumulate / invert / insert, the one-lane kernel compiled for
two waves per SIMD at n = 10): per observation and bit for bit against the
oracle's device-spec variant (B, pre-absorption state, flags, uniforms
consumed, fixed-point z, transition counts N), as tests/test_gpu_parity.py.

Every case names the conditions it is there for and FAILS when its inputs do
not reach them; the conditions that the oracle alone decides (jump counts,
rejected proposals) were checked on the CPU for the keys below.  Each oracle
result is computed once per (n, N) and shared by the cases that use it."""
import numpy as np
import pytest

import phasetype_amd as P
from phasetype_amd.synth import bd_exit, simulate_ph
from test_gpu_parity import _perturbed

pytestmark = pytest.mark.gpu

KEY, SWEEP = (0x51F0 + 3, 0x2B7E15), 5
_ORACLE = {}


def _case(orc, n, N):
    """exact observations only: BD-exit(n) data, perturbed parameters, the
    oracle's device-spec sweep (cached)"""
    if (n, N) not in _ORACLE:
        S0, s0 = bd_exit(n)
        y, cen = simulate_ph(S0, s0, N, seed=8100 + 7 * n + N, censor_frac=0.0)
        S, s = _perturbed(n, 40 + n)
        zexp = int(orc.lib.orc_zexp(np.ascontiguousarray(y), len(y)))
        o = orc.dev_sweep(2, S, s, y, cen, key=KEY, sweep=SWEEP, zexp=zexp)
        _ORACLE[(n, N)] = (S, s, y, cen, zexp, o)
    return _ORACLE[(n, N)]


def _jumps(o):
    """jumps per observation: its transition counts hold them plus the absorption"""
    return o["N"].sum(axis=(1, 2)) - 1


def _rejections(o, n):
    """rejected ARMS proposals of the whole sweep, from the oracle's density
    evaluations: a jump with r rejections evaluates 4 (initial envelope) + 1
    (f at xprev) + r + 1 times (the rare XEPS re-evaluations add to it)"""
    return int(o["stats"][0]) - 6 * int(_jumps(o).sum())


def _check(g, o, st, n, N):
    for f in ("B", "pre", "flags", "ndraw"):
        bad = np.nonzero(g[f] != o[f])[0]
        assert bad.size == 0, f"{f} differs at obs {bad[:5]}: gpu {g[f][bad[:5]]} oracle {o[f][bad[:5]]}"
    bad = np.nonzero(np.any(g["zq"] != o["zq"], axis=1))[0]
    assert bad.size == 0, f"zq differs at obs {bad[:5]}"
    bad = np.nonzero(np.any(g["N"] != o["N"], axis=(1, 2)))[0]
    assert bad.size == 0, f"N differs at obs {bad[:5]}"
    # the timed (non-debug) kernel: its statistics block against the oracle's totals
    zq, B, Nt, ex = P.split_stats(st, n)
    assert np.array_equal(zq, o["zq_tot"]) and np.array_equal(B, o["B_tot"]) and np.array_equal(Nt, o["N_tot"])
    assert ex[0] == N  # every observation sampled


def _run(orc, n, N):
    S, s, y, cen, zexp, o = _case(orc, n, N)
    sw = P.Sweeper(n, 2, 1)
    sw.set_obs(y, cen)
    g = sw.sweep_debug(S, s, key=KEY, sweep=SWEEP, zexp=zexp)
    st = sw.sweep(S, s, key=KEY, sweep=SWEEP, zexp=zexp)
    sw.close()
    _check(g, o, st, n, N)
    return o


@pytest.mark.parametrize("newcap", ["1", "0", "2"])
@pytest.mark.parametrize("N", [2048, 300])
@pytest.mark.parametrize("n", [3, 5, 10])
def test_onelane_round_newcap(gpu, orc, monkeypatch, n, N, newcap):
    """The one-lane kernel alone (no rows), PHT_NEWCAP = 1 (default), 0 and 2.
    N = 2048: lanes take several observations in turn; N = 300: fewer than the
    lanes of the blocks that share them, so most lanes never get one and a
    wave's last lanes start observations while none of it has a sojourn due.
    Conditions: observations absorbed at their first test (no jump: the test
    folded into the round), observations with two or more jumps (the absorb
    test of phase A failing, then succeeding) and rejected proposals (pending
    lanes: the insert and the converged blocks at 11 points)."""
    monkeypatch.setenv("PHT_ROWK", "0")
    monkeypatch.setenv("PHT_NEWCAP", newcap)
    o = _run(orc, n, N)
    j = _jumps(o)
    assert (j == 0).sum() > 0 and (j >= 2).sum() > 0, (int((j == 0).sum()), int((j >= 2).sum()))
    assert _rejections(o, n) > 0


@pytest.mark.parametrize("spread", ["1", "0"])
def test_onelane_round_spread(gpu, orc, monkeypatch, spread):
    """PHT_SPREAD=1 (lane-major first claims) and 0 at n = 10: the same
    observations in another lane order, the same per-observation results."""
    monkeypatch.setenv("PHT_ROWK", "0")
    monkeypatch.setenv("PHT_SPREAD", spread)
    o = _run(orc, 10, 2048)
    assert _rejections(o, 10) > 0


def test_round_with_rows(gpu, orc, monkeypatch):
    """Rows enabled at n = 10: the 64 longest observations on 16-lane rows
    (the kernel's ROWS instantiation, whose one-lane blocks run the same
    round code), the others one per lane."""
    monkeypatch.setenv("PHT_ROWK", "64")
    o = _run(orc, 10, 2048)
    assert (_jumps(o) >= 2).sum() > 64


_LONG_KEYS = [((5, 6), 2), ((3, 4), 1), ((9, 1), 7), ((11, 12), 3), ((21, 8), 9), ((2, 99), 4)]


def test_longest_256_of_20000(gpu, orc, monkeypatch):
    """The 256 longest of 20,000 simulated paths at n = 10, one per lane:
    many rounds per lane (the median path has at least 10 jumps), and rejection
    chains: the general ARMS continuation (an envelope beyond 13 points, i.e.
    a third rejection in one jump) must be seen at least once, which that
    lane reaches only through a pending round at 11 points and one at 13.
    (key, sweep) pairs are run until it has been (at most six)."""
    monkeypatch.setenv("PHT_ROWK", "0")
    n = 10
    S0, s0 = bd_exit(n)
    y, cen = simulate_ph(S0, s0, 20000, seed=4243)
    idx = np.sort(np.argsort(-y)[:256])
    y, cen = np.ascontiguousarray(y[idx]), np.ascontiguousarray(cen[idx])
    zexp = int(orc.lib.orc_zexp(y, len(y)))
    sw = P.Sweeper(n, 2, 1)
    sw.set_obs(y, cen)
    general = 0
    for key, sweep in _LONG_KEYS:
        o = orc.dev_sweep(2, S0, s0, y, cen, key=key, sweep=sweep, zexp=zexp)
        g = sw.sweep_debug(S0, s0, key=key, sweep=sweep, zexp=zexp)
        st = sw.sweep(S0, s0, key=key, sweep=sweep, zexp=zexp)
        _check(g, o, st, n, len(y))
        assert np.median(_jumps(o)) >= 10 and _jumps(o).min() >= 2, (float(np.median(_jumps(o))), int(_jumps(o).min()))
        general += int(P.split_stats(g["stats"], n)[3][P.XDBG_GENERAL])
        if general > 0:
            break
    sw.close()
    assert general > 0
