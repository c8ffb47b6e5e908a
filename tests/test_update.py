"""CPU: the conjugate update (step 2 of a sweep) on tied and scaled structures.

* The numpy statement of tests/update_cases.py against the oracle's Gibbs
  driver, one step at a time and bit for bit, on every structure, for the
  host-update chain (dev 1: the R stream's rgamma after the two key uniforms)
  and the resident chain (dev 2: the counter stream of include/pht_gamma.h).
* The oracle chains' draws against the closed-form posteriors (Kolmogorov-
  Smirnov, p > 1e-4 as tests/test_resident.py), and against three wrong laws
  (p < 1e-10 each).
* The oracle's UNIF chain on fr3 against the posterior computed by quadrature,
  within K_SIGMA batch-means MCSEs of the chain alone; the same chain against
  the posterior of the data scaled by 1.05 must miss by more than 8.
GPU: tests/test_gpu_update.py."""
import numpy as np
import pytest

import update_cases as UC
from oracle import posterior as PO

def _flat(M):
    return np.ascontiguousarray(np.asarray(M).reshape(-1, order="F"))


def _chain(orc, dev, it, method, c, y, cen, seed, start=None):
    orc.set_seed(seed)
    return orc.gibbs(dev, it, 1, method, c.n, c.nu, c.zeta, _flat(c.T).astype(np.int32), _flat(c.C), y, cen,
                     start=start)


def replay(orc, dev, it, method, c, y, cen, seed):
    """The chain rebuilt from update_cases: the oracle gives only the step-1
    statistics (dev_sweep) and the Gamma streams"""
    orc.set_seed(seed)
    key = (int(orc.lib.orc_unif_rand() * 4294967296.0), int(orc.lib.orc_unif_rand() * 4294967296.0))
    zexp = int(orc.lib.orc_zexp(np.ascontiguousarray(y), len(y)))

    def draw(k, i, a, scale):
        return orc.lib.orc_rgamma(a, scale) if dev == 1 else orc.rgamma_ctr_at(key, k, i, a, scale)

    rows = [np.array([(c.nu[k] - 1.0) / c.zeta[k] if c.nu[k] > 1 else draw(k, 0, c.nu[k], 1.0 / c.zeta[k])
                      for k in range(c.m)])]
    for i in range(1, it):
        S, s = UC.assemble(rows[-1], c.T, c.C, first=(i == 1))
        st = orc.dev_sweep(method, S, s, y, cen, key=key, sweep=i, zexp=zexp, per_obs=False)
        shape, scale = UC.update_args(c.T, c.C, c.nu, c.zeta, st["zq_tot"], st["N_tot"], zexp)
        rows.append(np.array([draw(k, i, shape[k], scale[k]) for k in range(c.m)]))
    return np.array(rows)


# dev 2's ECS / DCS sweeps run on the resident eigensystem, warm-started from
# the sweep before, which dev_sweep alone does not restate: the resident
# update is replayed under the samplers that need no eigensystem
STEP_CASES = [(name, meth, dev) for name, c in UC.CASES.items() for dev in (1, 2)
              for meth in c.samplers if meth in ((UC.UNIF, UC.ECS) if dev == 1 else (UC.UNIF,))]


@pytest.mark.parametrize("name,method,dev", STEP_CASES,
                         ids=[f"{n}-{UC.SAMPLER_NAMES[m]}-dev{d}" for n, m, d in STEP_CASES])
def test_numpy_statement_is_the_oracles_update(orc, name, method, dev):
    c = UC.CASES[name]
    y, cen = c.data(200, c.censor_frac(method))
    want = _chain(orc, dev, 4, method, c, y, cen, seed=77)
    got = replay(orc, dev, 4, method, c, y, cen, seed=77)
    assert np.array_equal(got, want), (got, want)


@pytest.mark.parametrize("dev", [1, 2])
@pytest.mark.parametrize("name,method", UC.LAW_CASES, ids=[n for n, _ in UC.LAW_CASES])
def test_closed_form_laws_oracle(orc, name, method, dev):
    c = UC.CASES[name]
    y, cen = UC.law_data(name)
    chain = _chain(orc, dev, UC.LAW_DRAWS + 1, method, c, y, cen, seed=4321 + dev)
    UC.check_laws(name, chain, y, cen)
    if name.startswith("erlang3c") or name.startswith("exp1c"):
        assert UC.wrong_laws(name, y, cen)["times_c"] is not None


def test_quadrature_is_anchored_to_mpmath():
    """the likelihood under the quadrature at three grid points against mpmath"""
    for censored in (False, True):
        y, cen = UC.fr3_data(censored)
        t = UC.fr3_posterior(y, cen)
        lo, hi = t["box"]
        pts = [(t["q50"][0], t["q50"][1]), (lo[0] * 1.01, hi[1] * 0.99), (hi[0] * 0.99, lo[1] * 1.01)]
        worst = UC.fr3_anchor(y, cen, pts)
        print(f"censored {censored}: G = {t['G']}, last move {t['last_move']:.2e}, edge {t['edge_mass']:.1e}, "
              f"|numpy - mpmath| = {worst:.2e}")
        assert worst < 1e-9, worst


@pytest.mark.parametrize("censored", [False, True], ids=["exact", "cens30"])
def test_quadrature_posterior_oracle_unif(orc, censored):
    c = UC.CASES["fr3"]
    y, cen = UC.fr3_data(censored)
    chain = _chain(orc, 1, UC.FR3_SWEEPS, UC.UNIF, c, y, cen, seed=99)
    UC.check_posterior(PO.summarize(chain[:, :2]), y, cen, PO.K_SIGMA, f"oracle UNIF censored={censored}")
