"""GPU: the conjugate update on tied and scaled structures (tests/update_cases.py),
through both implementations: GibbsState behind Sweeper.gibbs / LJMA_Gibbs /
gibbs_chains, and resident_update_kernel behind Sweeper.gibbs_resident.

* Bit-exact chains against the oracle (dev 1 / dev 2), every structure x
  admitted sampler; full9 (m = 81) takes the update kernel's loop round twice.
* One step without the oracle: rows 1 and 2 of a host-loop chain are the
  library's own R stream applied to update_cases.update_args of the library's
  own sweep statistics; likewise the resident chain with the counter stream.
* Resident chains under the cases' own priors (fr3c, bd10t), where the order
  of the kernel's zl walk reaches the draws.
* The closed-form laws and the quadrature posterior of fr3, as on the CPU
  (tests/test_update.py), for the host loop and the resident chain.
* The refusals of ParamLists::build through the three entry points."""
import numpy as np
import pytest

import phasetype_amd as P
import update_cases as UC
from oracle import posterior as PO

pytestmark = pytest.mark.gpu

N_BIT, IT_BIT = 1500, 25


def _flat(M):
    return np.ascontiguousarray(np.asarray(M).reshape(-1, order="F"))


def _sweeper(c, method, y, cen):
    sw = P.Sweeper(c.n, method, 1)
    sw.set_obs(y, cen)
    return sw


@pytest.mark.parametrize("name,method", UC.PAIRS, ids=UC.PAIR_IDS)
def test_chains_bitexact(gpu, orc, name, method):
    c = UC.CASES[name]
    y, cen = c.data(N_BIT, c.censor_frac(method))
    zexp = P.zexp_for(y)
    nu, zeta = c.tight_priors(y)
    sw = _sweeper(c, method, y, cen)
    for dev, run in ((1, sw.gibbs), (2, sw.gibbs_resident)):
        orc.set_seed(606)
        want = orc.gibbs(dev, IT_BIT, 1, method, c.n, nu, zeta, _flat(c.T).astype(np.int32), _flat(c.C), y, cen)
        P.set_seed(606)
        got = run(IT_BIT, method, nu, zeta, c.T, c.C, zexp)
        assert np.array_equal(got, want), (dev, np.argwhere(got != want)[:4], np.abs(got - want).max())
    sw.close()


# the cases' own (weak) priors keep every bit of zsum in the draw's scale, so a forward walk of the lists shows:
# on the oracle it changes 3 of fr3c's 48 draw arguments and bd10t's from sweep 1 on.  bd10t stops at 6 sweeps:
# under these priors z / c carries its chain to where UNIF's table overflows at sweep 12 (and MHRS crawls at its
# cap on both, so it is left to the tight-prior chains)
ORDER_CHAINS = [("fr3c", 25), ("bd10t", 6)]


@pytest.mark.parametrize("method", [UC.ECS, UC.UNIF], ids=["ECS", "UNIF"])
@pytest.mark.parametrize("name,it", ORDER_CHAINS, ids=[n for n, _ in ORDER_CHAINS])
def test_resident_chain_case_priors_bitexact(gpu, orc, name, it, method):
    c = UC.CASES[name]
    y, cen = c.data(N_BIT, 0.3)
    sw = _sweeper(c, method, y, cen)
    orc.set_seed(707)
    want = orc.gibbs(2, it, 1, method, c.n, c.nu, c.zeta, _flat(c.T).astype(np.int32), _flat(c.C), y, cen)
    P.set_seed(707)
    got = sw.gibbs_resident(it, method, c.nu, c.zeta, c.T, c.C, P.zexp_for(y))
    sw.close()
    assert np.array_equal(got, want), (np.argwhere(got != want)[:4], np.abs(got - want).max())


@pytest.mark.parametrize("name", ["fr3c", "bd10t"])
def test_resident_step_against_the_numpy_statement(gpu, orc, lib, name):
    """rows 1 and 2 of a resident chain are the counter stream's Gamma draws
    at update_args of the library's own sweep statistics (UNIF: the resident
    ECS / DCS sweeps run on the device's eigensystem, which sweep() does not)"""
    method = UC.UNIF
    c = UC.CASES[name]
    y, cen = c.data(N_BIT, 0.3)
    zexp = P.zexp_for(y)
    start = c.truth * np.linspace(0.9, 1.1, c.m)
    sw = _sweeper(c, method, y, cen)
    P.set_seed(808)
    got = sw.gibbs_resident(3, method, c.nu, c.zeta, c.T, c.C, zexp, start=start)
    assert np.array_equal(got[0], start)
    P.set_seed(808)
    key = (int(lib.pht_unif_rand() * 4294967296.0), int(lib.pht_unif_rand() * 4294967296.0))
    prev = start
    for i in (1, 2):
        S, s = UC.assemble(prev, c.T, c.C, first=(i == 1))
        zq, _, N, _ = P.split_stats(sw.sweep(S, s, key=key, sweep=i, zexp=zexp), c.n)
        shape, scale = UC.update_args(c.T, c.C, c.nu, c.zeta, zq, N, zexp)
        want = np.array([orc.rgamma_ctr_at(key, k, i, shape[k], scale[k]) for k in range(c.m)])
        assert np.array_equal(got[i], want), (i, got[i], want)
        prev = want
    sw.close()


def test_entry_points_agree(gpu):
    """LJMA_Gibbs and gibbs_chains give Sweeper.gibbs's chain (fr3c, ECS)"""
    c = UC.CASES["fr3c"]
    y, cen = c.data(N_BIT, 0.3)
    it, single = 12, []
    for seed in (11, 12):
        P.set_seed(seed)
        sw = _sweeper(c, UC.ECS, y, cen)
        single.append(sw.gibbs(it, UC.ECS, c.nu, c.zeta, c.T, c.C, P.zexp_for(y)))
        sw.close()
    P.set_seed(11)
    out = P.LJMA_Gibbs(it, 1, UC.ECS, c.n, c.m, c.nu, c.zeta, c.T, c.C, y, len(y), cen, [-1.0], 1, np.zeros(it * c.m))
    assert np.array_equal(out["res"].reshape(c.m, it).T, single[0])
    draws, _ = P.gibbs_chains([11, 12], y, cen, c.n, UC.ECS, c.nu, c.zeta, c.T, c.C, it=it)
    assert np.array_equal(draws[0], single[0]) and np.array_equal(draws[1], single[1])


@pytest.mark.parametrize("name", ["fr3c", "bd10t"])
@pytest.mark.parametrize("method", [UC.ECS, UC.UNIF], ids=["ECS", "UNIF"])
def test_one_step_without_the_oracle(gpu, lib, name, method):
    c = UC.CASES[name]
    y, cen = c.data(N_BIT, 0.3)
    zexp = P.zexp_for(y)
    start = c.truth * np.linspace(0.9, 1.1, c.m)
    sw = _sweeper(c, method, y, cen)
    P.set_seed(909)
    got = sw.gibbs(3, method, c.nu, c.zeta, c.T, c.C, zexp, start=start)
    assert np.array_equal(got[0], start)
    P.set_seed(909)
    key = (int(lib.pht_unif_rand() * 4294967296.0), int(lib.pht_unif_rand() * 4294967296.0))
    prev = start
    for i in (1, 2):
        S, s = UC.assemble(prev, c.T, c.C, first=(i == 1))
        zq, _, N, _ = P.split_stats(sw.sweep(S, s, key=key, sweep=i, zexp=zexp), c.n)
        shape, scale = UC.update_args(c.T, c.C, c.nu, c.zeta, zq, N, zexp)
        want = np.array([lib.pht_rgamma(shape[k], scale[k]) for k in range(c.m)])
        assert np.array_equal(got[i], want), (i, got[i], want)
        prev = want
    sw.close()


@pytest.mark.parametrize("path", ["host", "resident"])
@pytest.mark.parametrize("name,method", UC.LAW_CASES, ids=[n for n, _ in UC.LAW_CASES])
def test_closed_form_laws(gpu, name, method, path):
    c = UC.CASES[name]
    y, cen = UC.law_data(name)
    sw = _sweeper(c, method, y, cen)
    P.set_seed(2468)
    run = sw.gibbs if path == "host" else sw.gibbs_resident
    chain = run(UC.LAW_DRAWS + 1, method, c.nu, c.zeta, c.T, c.C, P.zexp_for(y))
    assert sw.flagged_obs == 0
    sw.close()
    UC.check_laws(name, chain, y, cen)


POSTERIOR = [(m, cens) for cens in (False, True) for m in (UC.ECS, UC.DCS, UC.UNIF) if not (cens and m == UC.DCS)]


@pytest.mark.parametrize("path", ["host", "resident"])
@pytest.mark.parametrize("method,censored", POSTERIOR,
                         ids=[f"{UC.SAMPLER_NAMES[m]}-{'cens30' if c else 'exact'}" for m, c in POSTERIOR])
def test_quadrature_posterior(gpu, method, censored, path):
    c = UC.CASES["fr3"]
    y, cen = UC.fr3_data(censored)
    sw = _sweeper(c, method, y, cen)
    P.set_seed(1357)
    run = sw.gibbs if path == "host" else sw.gibbs_resident
    chain = run(UC.FR3_SWEEPS, method, c.nu, c.zeta, c.T, c.C, P.zexp_for(y))
    assert sw.flagged_obs == 0
    sw.close()
    UC.check_posterior(PO.summarize(chain[:, :2]), y, cen, PO.K_SIGMA, f"{path} {UC.SAMPLER_NAMES[method]} censored={censored}")


def test_bad_structures_are_refused(gpu):
    """a cell in the absorbing row and a zero multiplier raise from every entry
    point, and the context runs a valid chain afterwards"""
    c = UC.CASES["fr3c"]
    y, cen = c.data(300, 0.3)
    zexp = P.zexp_for(y)
    Trow = c.T.copy()
    Trow[c.n, 0] = 1
    Czero = c.C.copy()
    Czero[0, 2] = 0.0
    sw = _sweeper(c, UC.ECS, y, cen)
    for T, C, why in ((Trow, c.C, r"T\[3,0\].*absorbing row"), (c.T, Czero, r"C\[0,2\].*not finite and > 0")):
        with pytest.raises(P.PhaseTypeError, match=why):
            sw.gibbs(4, UC.ECS, c.nu, c.zeta, T, C, zexp)
        with pytest.raises(P.PhaseTypeError, match=why):
            sw.gibbs_resident(4, UC.ECS, c.nu, c.zeta, T, C, zexp)
        with pytest.raises(P.PhaseTypeError, match=why):
            P.gibbs_chains([1, 2], y, cen, c.n, UC.ECS, c.nu, c.zeta, T, C, it=4)
    P.set_seed(5)
    a = sw.gibbs(6, UC.ECS, c.nu, c.zeta, c.T, c.C, zexp)
    P.set_seed(5)
    b = sw.gibbs(6, UC.ECS, c.nu, c.zeta, c.T, c.C, zexp)
    assert np.array_equal(a, b) and np.all(np.isfinite(a)) and np.all(a > 0)
    sw.close()
