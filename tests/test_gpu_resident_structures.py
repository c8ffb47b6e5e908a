"""GPU: the device-resident chain's eigensystem (include/pht_eigen.h over one
workgroup in resident_update_kernel) off birth-death structure
(tests/resident_cases.py), against the oracle's serial run of the same header
(gibbs dev = 2), bit for bit; tests/test_eigen_structures.py pins that serial
run to mpmath.

* Chains on acyclic (Coxian and general), dense symmetric-tied and stiffly
  scaled structures up to n = 32 (kMaxN, the LDS arrays full), ECS with 30 %
  censoring and DCS on exact data: 25 sweeps, tight priors, seed 606, as
  test_gpu_update.test_chains_bitexact.
* The warm start: four 60-sweep chains under weak priors in which the
  refinement is accepted on every sweep (symtied4) and declined on some, so
  that the full QR follows it (coxian4, coxian8, symtied8); the CPU test
  counts both paths along these very chains.
* Refusals, as error codes: a defective S at init (erlang3, erlang3c), the
  n = 32 Coxian whose eigenvectors do not reproduce it, a complex spectrum at
  init (ring) and mid-chain (cycle3: before and past the host's 256-sweep
  poll of the error word).  After each the same context runs a valid chain.
"""
import time

import numpy as np
import pytest

import phasetype_amd as P
import resident_cases as RC
import update_cases as UC

pytestmark = pytest.mark.gpu

N_BIT, N_BIT32, IT_BIT, SEED = 1500, 600, 25, 606
STRUCTURES = RC.chain_structures()


def _flat(M):
    return np.ascontiguousarray(np.asarray(M).reshape(-1, order="F"))


def _oracle_chain(orc, c, it, method, nu, zeta, y, cen, seed, start=None):
    """(chain, flagged observation-sweeps) of the oracle's resident chain"""
    orc.lib.orc_dev_flagged_count()
    orc.set_seed(seed)
    want = orc.gibbs(2, it, 1, method, c.n, nu, zeta, _flat(c.T).astype(np.int32), _flat(c.C), y, cen, start=start)
    return want, orc.lib.orc_dev_flagged_count()


def _check_chain(orc, sw, c, it, method, nu, zeta, y, cen, seed):
    want, flagged = _oracle_chain(orc, c, it, method, nu, zeta, y, cen, seed)
    assert np.all(np.isfinite(want))
    P.set_seed(seed)
    got = sw.gibbs_resident(it, method, nu, zeta, c.T, c.C, P.zexp_for(y))
    assert np.array_equal(got, want), (np.argwhere(got != want)[:4], np.abs(got - want).max())
    if flagged == 0:
        assert sw.flagged_obs == 0


@pytest.mark.parametrize("method", [UC.ECS, UC.DCS], ids=["ECS", "DCS"])
@pytest.mark.parametrize("name,built", STRUCTURES, ids=[n for n, _ in STRUCTURES])
def test_structure_chains_bitexact(gpu, orc, name, built, method):
    c = RC.case(name, built)
    y, cen = c.data(N_BIT32 if c.n == 32 else N_BIT, c.censor_frac(method))
    nu, zeta = c.tight_priors(y)
    sw = P.Sweeper(c.n, method, 1)
    sw.set_obs(y, cen)
    _check_chain(orc, sw, c, IT_BIT, method, nu, zeta, y, cen, SEED)
    sw.close()


@pytest.mark.parametrize("name,built", RC.warm_structures(), ids=[n for n, _ in RC.warm_structures()])
def test_warm_start_chains_bitexact(gpu, orc, name, built):
    c = RC.case(name, built)
    y, cen = c.data(RC.WARM_N, 0.3)
    sw = P.Sweeper(c.n, UC.ECS, 1)
    sw.set_obs(y, cen)
    _check_chain(orc, sw, c, RC.WARM_IT, UC.ECS, c.nu, c.zeta, y, cen, RC.WARM_SEED)
    sw.close()


def _usable_afterwards(orc, sw, c, method, y, cen):
    """the context that refused runs a valid chain of the same n, bit for bit"""
    nu, zeta = c.tight_priors(y)
    _check_chain(orc, sw, c, 8, method, nu, zeta, y, cen, SEED)


@pytest.mark.parametrize("method", [UC.ECS, UC.DCS], ids=["ECS", "DCS"])
@pytest.mark.parametrize("name", ["erlang3", "erlang3c"])
def test_defective_start_is_refused(gpu, orc, name, method):
    c = UC.CASES[name]
    y, cen = c.data(N_BIT, c.censor_frac(method))
    nu, zeta = c.tight_priors(y)
    sw = P.Sweeper(c.n, method, 1)
    sw.set_obs(y, cen)
    with pytest.raises(P.PhaseTypeError, match="eigensystem"):
        sw.gibbs_resident(IT_BIT, method, nu, zeta, c.T, c.C, P.zexp_for(y))
    _usable_afterwards(orc, sw, UC.CASES["fr3c"], method, y, cen)
    sw.close()


@pytest.mark.parametrize("name,built", [("coxian32", RC.coxian(RC.RAMP_N)), ("ring8", RC.ring(8))], ids=["coxian32", "ring8"])
def test_unusable_eigensystem_at_init_is_refused(gpu, orc, name, built):
    c = RC.case(name, built)
    y, cen = c.data(N_BIT32, 0.3)
    nu, zeta = c.tight_priors(y)
    sw = P.Sweeper(c.n, UC.ECS, 1)
    sw.set_obs(y, cen)
    with pytest.raises(P.PhaseTypeError, match="eigensystem"):
        sw.gibbs_resident(IT_BIT, UC.ECS, nu, zeta, c.T, c.C, P.zexp_for(y))
    good = RC.case(f"symtied{c.n}", RC.symtied(c.n))
    _usable_afterwards(orc, sw, good, UC.ECS, y, cen)
    sw.close()


@pytest.mark.parametrize("it", [6, 300])
def test_mid_chain_failure_is_refused(gpu, orc, it):
    """cycle3 turns complex at sweep 1: the later update kernels return at
    entry, and past 256 sweeps the host's poll of the error word stops the
    enqueueing.  The same error either way, and at once."""
    c = RC.case("cycle3", RC.cycle3())
    y, cen = c.data(N_BIT, 0.3)
    nu, zeta = RC.cycle3_priors(y)
    sw = P.Sweeper(c.n, UC.ECS, 1)
    sw.set_obs(y, cen)
    t0 = time.perf_counter()
    with pytest.raises(P.PhaseTypeError, match="eigensystem"):
        sw.gibbs_resident(it, UC.ECS, nu, zeta, c.T, c.C, P.zexp_for(y), start=np.array(RC.CYCLE3_START))
    assert time.perf_counter() - t0 < 1.0
    _usable_afterwards(orc, sw, UC.CASES["fr3c"], UC.ECS, y, cen)
    sw.close()
