"""GPU: the HIP kernels sample the right conditional path law off BD-exit.

The cases of tests/pathlaw_ref.py's table, in the same layout and under the
same keys as tests/test_pathlaw.py runs them through the device
specification, here on the kernels' own per-observation record
(``Sweeper.sweep_debug``): the bookkeeping invariants of every path, every
(y, censoring) group's means within 5 standard errors of the exact
conditional expectations, the censored groups' residual life.  The oracle is
not called: a mistake shared by a kernel and its restatement fails here.  As
kernels and specification agree bit for bit per observation, each case's
printed worst z-score equals the CPU file's; a difference is a parity break.

The production launch (``Sweeper.sweep``) must give the debug launch's block,
and per sampler family its blocks over 16 keys are compared with the summed
truths (tests/test_gpu_estep.py's check of BD-exit(4), on reversible 5)."""
import numpy as np
import pytest

import pathlaw_ref as PL
import phasetype_amd as P
from oracle.posterior import K_SIGMA

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", [c["name"] for c in PL.CASES])
def test_gpu_path_law(gpu, monkeypatch, name):
    case = PL.CASE_BY_NAME[name]
    for k, v in case["env"].items():  # read when the context is created
        monkeypatch.setenv(k, v)
    n = case["n"]
    S, s, lay, truths = PL.inputs(case)
    y, cen = lay[0], lay[1]
    zexp = P.zexp_for(y)
    sw = P.Sweeper(n, case["method"], case["mhit"])
    sw.set_obs(y, cen)
    g = sw.sweep_debug(S, s, key=case["key"], sweep=case["sweep"], zexp=zexp)
    st = sw.sweep(S, s, key=case["key"], sweep=case["sweep"], zexp=zexp)
    sw.close()
    g["zexp"] = zexp
    res = PL.check_record(g, case, S, s, lay, truths)
    print(PL.report(case, res))
    assert not res["violations"], res["violations"]
    assert res["worst"] <= K_SIGMA, (name, np.round(res["z"]["z"], 2), np.round(res["z"]["N"], 2))
    assert res["resid"] <= 5.0, (name, res["resid"])
    # the production launch: the debug launch's block, every observation counted
    assert np.array_equal(st[:2 * n + n * n], g["stats"][:2 * n + n * n])
    assert P.split_stats(st, n)[3][0] == len(y)
    zq, _, Nt, _ = P.split_stats(st, n)
    assert np.array_equal(zq, g["zq"].sum(0)) and np.array_equal(Nt, g["N"].sum(0, dtype=np.int64))
    if case["general"]:  # the tail groups ran the general ARMS code (counted by the one-lane debug launch)
        ex = P.split_stats(g["stats"], n)[3]
        print(f"pathlaw {name}: general ARMS rounds {int(ex[P.XDBG_GENERAL])}, "
              f"private envelope {int(ex[P.XDBG_PRIVATE])}")
        assert ex[P.XDBG_GENERAL] > 0


@pytest.mark.parametrize("family", ["ecs", "dcs", "unif"])
def test_production_kernel_against_the_summed_truths(gpu, family):
    """Sweeper.sweep alone, 16 sweeps with distinct keys over the reversible-5
    layout (32000 observations, four times, exact and censored): every cell's
    sweep mean of z, N and exits within 5 standard errors (sweep-to-sweep
    spread, counts floored at the Poisson level) of the group truths' sum"""
    case = dict(PL.CASE_BY_NAME["ecs-reversible5"], method={"ecs": PL.ECS, "dcs": PL.DCS, "unif": PL.UNIF}[family])
    n, sweeps = case["n"], 16
    S, s, (y, cen, grp, pairs), truths = PL.inputs(case)
    want_z = case["R"] * sum(t[0] for t in truths)
    want_N = case["R"] * sum(t[1] for t in truths)
    zexp = P.zexp_for(y)
    sw = P.Sweeper(n, case["method"], 1)
    sw.set_obs(y, cen)
    zs, Ns = [], []
    for k in range(sweeps):
        zq, _, Nk, ex = P.split_stats(sw.sweep(S, s, key=(0x5800 + k, case["method"]), sweep=k + 1, zexp=zexp), n)
        assert ex[0] == len(y)
        zs.append(np.ldexp(zq.astype(np.float64), -zexp))
        Ns.append(Nk.astype(np.float64))
    sw.close()
    for nm, X, want, floor in (("z", np.array(zs), want_z, False), ("N", np.array(Ns), want_N, True)):
        mean, se = X.mean(0), X.std(0, ddof=1) / np.sqrt(sweeps)
        if floor:
            se = np.maximum(se, np.sqrt(want / sweeps))
        d = np.abs(mean - want)
        zsc = np.where(se > 0, d / np.where(se > 0, se, 1.0), np.where(d > 0, np.inf, 0.0))
        print(f"pathlaw production {family} {nm}: largest z-score {zsc.max():.2f}, "
              f"relative 5 se of that cell {5 * se.flat[np.argmax(zsc)] / want.flat[np.argmax(zsc)]:.2e}")
        assert np.all(zsc <= K_SIGMA), (family, nm, zsc)
