"""GPU: the ECS exact kernel's weighted dealing between the two blocks of a
CU (PHT_ECS_PAIR, phasetype_amd/csrc/pht_claim.h) changes no result: an
observation's outcome depends only on its id, the key, the sweep and the
parameters, and the statistics are int64 sums.  Knob on (4:3, and 3:2 where
the dealing is live) against PHT_ECS_PAIR=0 in the same library: the
per-observation debug outputs and the statistics block are equal bit for bit,
and every Gibbs sweep passes the processed-count check.

The dealing is live only for a grid of exactly two one-lane blocks per CU
with no rows and no spread (at least 512 x 256 observations' worth of blocks
on an MI355X: N = 200,003 with PHT_SPREAD=0 PHT_ROWK=0 gives every block
several chunks and a ragged last one); every other shape here falls back to
the stripes and must equally agree."""
import numpy as np
import pytest

import phasetype_amd as P
from phasetype_amd.synth import bd_exit, bd_exit_structure, simulate_ph

pytestmark = pytest.mark.gpu

KNOBS = ("PHT_ECS_PAIR", "PHT_SPREAD", "PHT_ROWK", "PHT_ECS_OCC", "PHT_PIPELINE", "PHT_NEWCAP")
LIVE = {"PHT_SPREAD": "0", "PHT_ROWK": "0"}
_data = {}


def data(n, N, censor=0.0):
    """(S, s, y, cen, zexp) of a shape, simulated once"""
    key = (n, N, censor)
    if key not in _data:
        S, s = bd_exit(n)
        y, cen = simulate_ph(S, s, N, seed=0xC1A1 + n, censor_frac=censor)
        _data[key] = (S, s, y, cen, P.zexp_for(y))
    return _data[key]


def set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def debug_sweep(monkeypatch, n, N, env, pair, censor=0.0, obs0=0):
    S, s, y, cen, zexp = data(n, N, censor)
    set_env(monkeypatch, dict(env, PHT_ECS_PAIR=str(pair)))
    sw = P.Sweeper(n, 2)
    try:
        sw.set_obs(y, cen, obs0=obs0)
        return sw.sweep_debug(S, s, key=(11, 12), sweep=3, zexp=zexp)
    finally:
        sw.close()


def same(a, b):
    for f in ("stats", "B", "pre", "flags", "ndraw", "zq", "N"):
        assert np.array_equal(a[f], b[f]), f


@pytest.mark.parametrize("n", [3, 10])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 4096])
def test_small_shapes(gpu, monkeypatch, n, N):
    same(debug_sweep(monkeypatch, n, N, {}, 0), debug_sweep(monkeypatch, n, N, {}, 43))


@pytest.fixture(scope="module")
def ref3():
    """n = 3, N = 200,003 on the stripes: shared by the cases below, unchanged"""
    mp = pytest.MonkeyPatch()
    try:
        return debug_sweep(mp, 3, 200_003, LIVE, 0)
    finally:
        mp.undo()


@pytest.mark.parametrize("pair", [43, 32])
def test_live_dealing_n3(gpu, monkeypatch, ref3, pair):
    got = debug_sweep(monkeypatch, 3, 200_003, LIVE, pair)
    assert int(got["stats"][2 * 3 + 9]) == 200_003  # kXObs: every observation once
    same(ref3, got)


def test_one_block_per_cu(gpu, monkeypatch, ref3):
    same(ref3, debug_sweep(monkeypatch, 3, 200_003, dict(LIVE, PHT_ECS_OCC="1"), 43))


def test_spread(gpu, monkeypatch, ref3):
    same(ref3, debug_sweep(monkeypatch, 3, 200_003, {"PHT_SPREAD": "1", "PHT_ROWK": "0"}, 43))


def test_shard_obs0(gpu, monkeypatch):
    a = debug_sweep(monkeypatch, 3, 200_003, LIVE, 0, obs0=1_000_003)
    same(a, debug_sweep(monkeypatch, 3, 200_003, LIVE, 43, obs0=1_000_003))


def test_rows_n10(gpu, monkeypatch):
    env = {"PHT_ROWK": "64", "PHT_SPREAD": "0"}
    same(debug_sweep(monkeypatch, 10, 4096, env, 0), debug_sweep(monkeypatch, 10, 4096, env, 43))


def test_censored_n10(gpu, monkeypatch):
    same(debug_sweep(monkeypatch, 10, 4096, {}, 0, censor=0.3), debug_sweep(monkeypatch, 10, 4096, {}, 43, censor=0.3))


def test_live_dealing_n10_statistics(gpu, monkeypatch):
    """the flagship kernel (n = 10, two waves per SIMD, two blocks per CU:
    tests/test_kernel_regs.py): its statistics block, timed launch"""
    S, s, y, cen, zexp = data(10, 200_003)
    out = []
    for pair in (0, 43, 32):
        set_env(monkeypatch, dict(LIVE, PHT_ECS_PAIR=str(pair)))
        sw = P.Sweeper(10, 2)
        sw.set_obs(y, cen)
        out.append(sw.sweep(S, s, key=(5, 6), sweep=2, zexp=zexp))
        sw.close()
    assert int(out[0][2 * 10 + 100]) == 200_003
    for o in out[1:]:
        assert np.array_equal(out[0], o)


def gibbs(monkeypatch, n, N, env, it):
    S, s, y, cen, zexp = data(n, N)
    T, theta = bd_exit_structure(n)
    nu, zeta = 1 + 50 * theta, np.full(len(theta), 50.0)
    set_env(monkeypatch, env)
    sw = P.Sweeper(n, 2)
    try:
        sw.set_obs(y, cen)
        sw.set_global_count(N)  # every sweep: the processed count must be N
        P.set_seed(9)
        return sw.gibbs(it, 2, nu, zeta, T, np.ones(T.shape), zexp)
    finally:
        sw.close()


def test_pipelined_loop(gpu, monkeypatch):
    """6 sweeps of the pipelined loop, dealing on and off, against the
    loop that enqueues each sweep after the last"""
    ref = gibbs(monkeypatch, 3, 200_003, dict(LIVE, PHT_ECS_PAIR="0", PHT_PIPELINE="0"), 7)
    assert np.array_equal(ref, gibbs(monkeypatch, 3, 200_003, dict(LIVE, PHT_ECS_PAIR="43"), 7))
    assert np.array_equal(ref, gibbs(monkeypatch, 3, 200_003, dict(LIVE, PHT_ECS_PAIR="43", PHT_PIPELINE="0"), 7))
    assert np.array_equal(ref, gibbs(monkeypatch, 3, 200_003, dict(LIVE, PHT_ECS_PAIR="0"), 7))


def test_two_chains_one_launch(gpu, monkeypatch):
    """the chains launch keeps the stripes: each chain equals its single run"""
    n, N = 3, 200_003
    S, s, y, cen, zexp = data(n, N)
    T, theta = bd_exit_structure(n)
    nu, zeta = 1 + 50 * theta, np.full(len(theta), 50.0)
    set_env(monkeypatch, dict(LIVE, PHT_ECS_PAIR="43"))
    draws, _ = P.gibbs_chains([9, 10], y, cen, n, 2, nu, zeta, T, np.ones(T.shape), it=3)
    for c, seed in enumerate((9, 10)):
        sw = P.Sweeper(n, 2)
        sw.set_obs(y, cen)
        P.set_seed(seed)
        one = sw.gibbs(3, 2, nu, zeta, T, np.ones(T.shape), zexp)
        sw.close()
        assert np.array_equal(draws[c], one)
