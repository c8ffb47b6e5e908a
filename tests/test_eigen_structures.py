"""CPU: the device-resident chain's eigensystem (include/pht_eigen.h, run
serially by the oracle) off birth-death structure, against a high-precision
truth, and its refusal of defective and nearly defective generators.
tests/test_gpu_resident_structures.py replays the chains of this file on the
HIP update kernel, bit for bit.

Accuracy.  Per case: rc 0, unit columns, the eigenvalues against mpmath.eig at
50 digits within 64 eps cond(Q) scale, and the quantity the samplers consume,
the row e_1^T Q exp(Lambda y) Q^-1 at y = 0.1 / mu, 1 / mu, 10 / mu, against
the first row of mpmath's expm (evaluator_cases._row), relative to the row's
largest entry.  The bar is that of tests/test_eigen.py, measured against what
the reference uses: err <= 8 x (the same error of numpy.linalg.eig + inv on the
same matrix) + 64 eps.

Observed (the header's error, LAPACK's, their ratio):

    case            header   LAPACK   ratio     case              header   LAPACK   ratio
    acyclic-4       4.5e-16  2.3e-16  2.00      bd-3              2.6e-15  2.1e-15  1.24
    acyclic-8       9.4e-14  5.6e-14  1.69      bd-10             2.4e-14  1.6e-14  1.51
    acyclic-12      2.0e-12  8.1e-12  0.25      bd-20             2.4e-11  1.6e-11  1.49
    acyclic-16      1.3e-14  1.1e-14  1.26      bd-32             8.0e-08  1.8e-07  0.45
    acyclic-20      1.7e-12  9.3e-13  1.81      truth-coxian4     8.6e-16  1.2e-15  0.73
    acyclic-32      8.8e-14  4.5e-14  1.98      truth-coxian8     4.8e-14  5.7e-14  0.84
    reversible-5    2.7e-15  7.5e-16  3.55      truth-coxian16    3.2e-11  2.2e-11  1.45
    reversible-10   9.7e-16  1.5e-15  0.64      truth-acyclic8    1.2e-14  1.2e-14  1.06
    reversible-15   1.8e-15  1.2e-15  1.46      truth-acyclic16   2.8e-15  4.6e-15  0.61
    reversible-20   1.7e-15  2.4e-15  0.71      truth-acyclic32   8.3e-13  8.8e-13  0.94
    reversible-32   2.1e-15  2.2e-15  0.98      truth-symtied5    2.2e-15  2.3e-15  0.94
    neareq-6        2.6e-08  2.4e-08  1.09      truth-symtied5c   2.4e-16  1.2e-16  2.00
    neareq-12       2.0e-08  3.3e-08  0.61      truth-symtied10   1.3e-15  3.9e-15  0.34
    neareq-32       7.4e-10  1.1e-09  0.64      truth-symtied10c  7.3e-16  4.9e-16  1.50
    stiff-6         1.1e-16  1.1e-16  1.00      truth-symtied32   4.1e-15  5.6e-15  0.73
    stiff-12        1.1e-16  1.1e-16  1.00      truth-symtied32c  7.4e-16  2.6e-16  2.88
    stiff-32        4.4e-16  3.6e-16  1.22      truth-cycle3      6.1e-16  1.1e-15  0.57
    hypoexp-3       1.1e-16  2.0e-16  0.52
    hypoexp-6       3.0e-15  2.6e-15  1.17
    hypoexp-10      9.0e-14  5.4e-14  1.66

The error of a case is its largest over the three y, on both sides.  Per y
the ratio can be far from 1 without either side being wrong: on
truth-coxian16 at y = 1 / mu the header is at 4.3e-12 and LAPACK at 9.7e-14,
while the two eigenvector matrices agree to one ulp per entry and the
header's inverse is the closer one to the 60-digit inverse (1.3e-14 against
1.6e-14 relative).  With the exact inverse of its own eigenvectors LAPACK
gives 2.2e-12 there too: numpy's inverse carries rounding correlated with its
V, which happens to cancel at that y and not at 10 / mu (3.2e-11, 2.2e-11).

Refusal (PHT_EIG_SINGULAR, 3, unless noted): rc != 0 for the exactly defective
chains (erlang, coxian_shared: n = 3, 6, 10, 32), the nearly defective ones
(gapped(3) at 1e-12, 1e-9, 1e-6; gapped(6) and gapped(10) at every eps) and
the two whose eigenvector matrices double precision cannot invert, hypoexp(32)
and the n = 32 Coxian ramp; rc 0 stays for gapped(3, 1e-3), neareq 6 / 12 / 32,
bd_exit(32) and hypoexp(10).  The residuals and their distance to the bound
are tabulated in DESIGN.md, section 7d.  Before the acceptance check
(pht_eig_verify) every one of the refused cases but erlang(32) and
coxian_shared(32) returned rc 0 with a Q diag(lambda) Q^-1 that is not S.

The oracle's resident chain (gibbs dev = 2) stops where the eigensystem
refuses: NaN rows after the last sweep whose S was refused.
"""
import os
import re

import numpy as np
import pytest

import evaluator_cases as EC
import resident_cases as RC
import test_gpu_structures as TS
import update_cases as UC
from phasetype_amd.synth import bd_exit

EPS = np.finfo(float).eps
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def _structure(kind, n):
    return TS.sweep_params(kind, *TS.generator(kind, n, 100 + n), 7 * n + 1)[0]


def _accuracy_cases():
    out = [(f"{kind}-{n}", (lambda kind=kind, n=n: _structure(kind, n)))
           for kind, ns in (("acyclic", (4, 8, 12, 16, 20, 32)), ("reversible", (5, 10, 15, 20, 32)), ("neareq", (6, 12, 32)))
           for n in ns]
    out += [(f"stiff-{n}", (lambda n=n: EC.stiff(n)[0])) for n in (6, 12, 32)]
    out += [(f"hypoexp-{n}", (lambda n=n: EC.hypoexp(n)[0])) for n in (3, 6, 10)]
    out += [(f"bd-{n}", (lambda n=n: bd_exit(n)[0])) for n in (3, 10, 20, 32)]
    out += [(f"truth-{name}", (lambda b=b: RC.generator(b)[0])) for name, b in RC.chain_structures()]
    out += [("truth-cycle3", lambda: RC.generator(RC.cycle3())[0])]
    return out


ACCURACY = _accuracy_cases()


def _row_error(S, lam, Q, Qi, y):
    """max |e_1^T Q exp(lam y) Q^-1 - first row of expm(S y)| / the row's largest entry"""
    import mpmath as mp

    want, dps = EC._row(np.ascontiguousarray(S, np.float64), y)
    with mp.workdps(dps):
        ref = np.array([float(v) for v in want])
    got = np.real((Q[0, :] * np.exp(lam * y)) @ Qi)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("name,make", ACCURACY, ids=[n for n, _ in ACCURACY])
def test_eig_against_high_precision(orc, name, make):
    import mpmath as mp

    S = np.ascontiguousarray(make(), np.float64)
    n = S.shape[0]
    rc, ev, Q, Qi = orc.eig(S)
    assert rc == 0
    assert np.allclose(np.linalg.norm(Q, axis=0), 1.0, rtol=1e-14)
    with mp.workdps(50):
        E, _ = mp.eig(mp.matrix(S.tolist()))
        assert max(abs(mp.im(e)) for e in E) < mp.mpf(10) ** -30
        want = np.sort(np.array([float(mp.re(e)) for e in E]))
    mu = float(np.abs(np.diag(S)).max())
    scale = float(np.abs(want).max())
    tol = 64 * EPS * np.linalg.cond(Q) * scale
    assert np.abs(np.sort(ev) - want).max() <= tol, (np.abs(np.sort(ev) - want).max(), tol)
    w, V = np.linalg.eig(S)
    Vi = np.linalg.inv(V)
    err = lap = 0.0
    for y in (0.1 / mu, 1.0 / mu, 10.0 / mu):
        e, l = _row_error(S, ev, Q, Qi, y), _row_error(S, w, V, Vi, y)
        print(f"{name}: y mu = {y * mu:g}: header {e:.2e}, LAPACK {l:.2e}")
        err, lap = max(err, e), max(lap, l)
    print(f"{name}: header {err:.1e} LAPACK {lap:.1e} ratio {err / lap:.2f}")
    assert err <= 8 * lap + 64 * EPS, (name, err, lap)


def _ramp():
    return RC.generator(RC.coxian(RC.RAMP_N))[0]


REFUSED = ([(f"{f}-{n}", (lambda f=f, n=n: EC.generator(f, n)[0])) for f in ("erlang", "coxian_shared") for n in (3, 6, 10, 32)]
           + [(f"gapped-3-{e:g}", (lambda e=e: EC.gapped(3, eps=e)[0])) for e in (1e-12, 1e-9, 1e-6)]
           + [(f"gapped-{n}-{e:g}", (lambda n=n, e=e: EC.gapped(n, eps=e)[0])) for n in (6, 10) for e in EC.EPS]
           + [("hypoexp-32", lambda: EC.hypoexp(32)[0]), ("coxian-ramp-32", _ramp)]
           + [(nm, (lambda nm=nm: UC.CASES[nm].generator()[0])) for nm in ("erlang3", "erlang3c")])
ACCEPTED = ([("gapped-3-0.001", lambda: EC.gapped(3, eps=1e-3)[0])]
            + [(f"neareq-{n}", (lambda n=n: _structure("neareq", n))) for n in (6, 12, 32)]
            + [("bd-32", lambda: bd_exit(32)[0]), ("hypoexp-10", lambda: EC.hypoexp(10)[0])])


def _residual(S, ev, Q, Qi):
    with np.errstate(all="ignore"):
        return float(np.abs(Q @ np.diag(ev) @ Qi - S).max() / np.abs(np.diag(S)).max())


@pytest.mark.parametrize("name,make", REFUSED, ids=[n for n, _ in REFUSED])
def test_defective_generators_are_refused(orc, name, make):
    S = make()
    rc, ev, Q, Qi = orc.eig(S)
    print(f"{name}: rc {rc}, residual / mu {_residual(S, ev, Q, Qi):.3g}")
    assert rc != 0


@pytest.mark.parametrize("name,make", ACCEPTED, ids=[n for n, _ in ACCEPTED])
def test_well_conditioned_generators_stay_accepted(orc, name, make):
    S = make()
    rc, ev, Q, Qi = orc.eig(S)
    r = _residual(S, ev, Q, Qi)
    print(f"{name}: rc {rc}, residual / mu {r:.3g}")
    assert rc == 0
    assert r <= EC.E_MAX


def test_refused_spectra_by_kind(orc):
    """the complex pairs are reported as such (rc 1), not as defective"""
    assert orc.eig(RC.generator(RC.ring(8))[0])[0] == 1
    T, C, _ = RC.cycle3()
    assert orc.eig(UC.assemble(RC.CYCLE3_START, T, C, True)[0])[0] == 0
    assert orc.eig(UC.assemble(RC.CYCLE3_TARGET, T, C, False)[0])[0] == 1


def test_tolerance_is_the_evaluators(orc):
    """PHT_EIG_RESID_TOL is PHT_LL_EMAX, the cancellation the spectral
    log-likelihood tolerates: one number in the project, not two"""
    eig = open(os.path.join(INCLUDE, "pht_eigen.h")).read()
    ll = open(os.path.join(INCLUDE, "pht_loglik.h")).read()
    tol = float.fromhex(re.search(r"#define PHT_EIG_RESID_TOL (\S+)", eig).group(1))
    assert tol == float.fromhex(re.search(r"#define PHT_LL_EMAX (\S+)", ll).group(1)) == EC.E_MAX


def test_refine_cannot_hand_out_what_the_qr_refuses(orc):
    """an accepted refinement passes the same check: started from the exact
    eigensystem of a neighbour, the nearly defective gapped(3, 1e-6) is
    refused or declined, never returned"""
    S0 = EC.gapped(3, eps=1e-3)[0]
    rc, ev, Q, Qi = orc.eig(S0)
    assert rc == 0
    for eps in (1e-6, 1e-9, 0.0):
        rc2, ev2, Q2, Qi2 = orc.eig_refine(EC.gapped(3, eps=eps)[0], Q, Qi)
        assert rc2 != 0, eps


# ------------------------------------------------------------ along the chains
def _flat(M):
    return np.ascontiguousarray(np.asarray(M).reshape(-1, order="F"))


@pytest.mark.parametrize("name,built", RC.warm_structures(), ids=[n for n, _ in RC.warm_structures()])
def test_warm_start_paths_along_the_chains(orc, name, built):
    """the weak-prior chains the GPU test replays take the refine-accepted
    path and the decline-then-QR path: no fallback on symtied4, some but not
    every sweep on the other three (observed: 0, and 51 / 58 / 36 of 59)"""
    c = RC.case(name, built)
    y, cen = c.data(RC.WARM_N, 0.3)
    orc.lib.orc_eig_fallback_count()
    orc.set_seed(RC.WARM_SEED)
    ch = orc.gibbs(2, RC.WARM_IT, 1, UC.ECS, c.n, c.nu, c.zeta, _flat(c.T).astype(np.int32), _flat(c.C), y, cen)
    fb = orc.lib.orc_eig_fallback_count()
    print(f"{name}: {fb} fallbacks in {RC.WARM_IT - 1} sweeps")
    assert np.all(np.isfinite(ch)) and np.all(ch > 0)
    if name == "symtied4":
        assert fb == 0
    else:
        assert 0 < fb < RC.WARM_IT - 1


@pytest.mark.parametrize("method", [UC.ECS, UC.DCS], ids=["ECS", "DCS"])
@pytest.mark.parametrize("name", ["erlang3", "erlang3c"])
def test_oracle_chain_stops_at_a_defective_start(orc, name, method):
    """erlang3(c) is defective at every parameter: the eigensystem of the
    start row is refused, sweep 0, and no row follows it"""
    c = UC.CASES[name]
    y, cen = c.data(300, c.censor_frac(method))
    nu, zeta = c.tight_priors(y)
    orc.set_seed(606)
    ch = orc.gibbs(2, 25, 1, method, c.n, nu, zeta, _flat(c.T).astype(np.int32), _flat(c.C), y, cen)
    assert np.all(np.isfinite(ch[0])) and np.all(np.isnan(ch[1:]))


def test_oracle_chain_stops_mid_chain(orc):
    """cycle3: real at the start, the first draw lands on the target, whose
    spectrum is complex: sweep 1 is the last row"""
    c = RC.case("cycle3", RC.cycle3())
    y, cen = c.data(RC.WARM_N, 0.3)
    nu, zeta = RC.cycle3_priors(y)
    orc.set_seed(606)
    ch = orc.gibbs(2, 25, 1, UC.ECS, c.n, nu, zeta, _flat(c.T).astype(np.int32), _flat(c.C), y, cen,
                   start=np.array(RC.CYCLE3_START))
    print("cycle3 row 1:", ch[1])
    assert np.array_equal(ch[0], RC.CYCLE3_START)
    assert np.allclose(ch[1], RC.CYCLE3_TARGET, rtol=1e-3)
    assert np.all(np.isnan(ch[2:]))
