"""The structures on which the device-resident chain's eigensystem
(include/pht_eigen.h) is tested off birth-death shape.  Shared by
tests/test_eigen_structures.py (CPU: the header, serial, against mpmath and
along the oracle's chains) and tests/test_gpu_resident_structures.py (the HIP
update kernel against the oracle's chains).  CPU only: no GPU and no oracle is
in it.

Every builder returns (T, C, truth) in the convention of update_cases._fill:
T[i, j] = k + 1 puts parameter k into cell (i, j) with multiplier C[i, j],
column n is the exit.  ``case`` wraps one into an update_cases.Case, whose
``data`` and ``tight_priors`` the chains use.

* ``coxian(n)``: the chain 0 -> 1 -> ... -> n - 1 with an exit from every state
  and a parameter per cell (m = 2n - 1): forward 1 + 0.3 i, exits 0.4 + 0.17 i,
  the last exit 2 + 0.3 (n - 1).  Acyclic: the spectrum is the diagonal, the
  total rates 1.4 + 0.47 i.  At n = 32 its eigenvector matrix is too
  ill-conditioned for double precision (the "ramp": refused).
* ``acyclic(n)``: a parameter per non-zero cell of
  test_gpu_structures.acyclic(n, 100 + n), the truth that generator's rates.
* ``symtied(n, scaled)``: one parameter per pair i < j, in both cells (i, j)
  and (j, i), and one per exit; multipliers d_i along row i (d = 1, or
  logspace(-1, 1, n)).  S = D A with A symmetric: the spectrum is real for
  every positive parameter, so no draw of the chain can turn it complex.
* ``cycle3()``: three states, parameter 1 round the cycle one way, parameter 2
  the other way, parameter 3 on the exits.  Symmetric (real spectrum) at
  CYCLE3_START, a complex pair at CYCLE3_TARGET, where ``cycle3_priors`` sends
  the first draw: the eigensystem fails mid-chain, at sweep 1.
* ``ring(n)``: one direction only with weak exits: complex from the start.
"""
import numpy as np

import update_cases as UC

COXIAN_N = (4, 8, 16)
ACYCLIC_N = (8, 16, 32)
SYMTIED_N = (5, 10, 32)
RAMP_N = 32
CYCLE3_START = (1.0, 1.0, 0.3)
CYCLE3_TARGET = (10.0, 0.01, 0.1)


def coxian(n):
    ent, truth = [], []
    for i in range(n - 1):
        truth.append(1.0 + 0.3 * i)
        ent.append((i, i + 1, len(truth), 1.0))
    for i in range(n):
        truth.append(0.4 + 0.17 * i if i < n - 1 else 2.0 + 0.3 * (n - 1))
        ent.append((i, n, len(truth), 1.0))
    T, C = UC._fill(n, ent)
    return T, C, np.array(truth)


def acyclic(n):
    import test_gpu_structures as TS

    S, s = TS.acyclic(n, 100 + n)
    G = np.concatenate([S, s[:, None]], axis=1)
    ent, truth = [], []
    for i in range(n):
        for j in range(n + 1):
            if j != i and G[i, j] != 0.0:
                truth.append(G[i, j])
                ent.append((i, j, len(truth), 1.0))
    T, C = UC._fill(n, ent)
    return T, C, np.array(truth)


def symtied(n, scaled=False):
    d = np.logspace(-1, 1, n) if scaled else np.ones(n)
    rng = np.random.default_rng(4)
    ent, truth = [], []
    for i in range(n):
        for j in range(i + 1, n):
            truth.append(float(rng.uniform(0.2, 1.0)) * 3.0 / n)
            ent += [(i, j, len(truth), float(d[i])), (j, i, len(truth), float(d[j]))]
    for i in range(n):
        truth.append(float(rng.uniform(0.1, 0.6)))
        ent.append((i, n, len(truth), float(d[i])))
    T, C = UC._fill(n, ent)
    return T, C, np.array(truth)


def cycle3():
    T, C = UC._fill(3, [(0, 1, 1, 1.0), (1, 2, 1, 1.0), (2, 0, 1, 1.0), (1, 0, 2, 1.0), (2, 1, 2, 1.0), (0, 2, 2, 1.0),
                        (0, 3, 3, 1.0), (1, 3, 3, 1.0), (2, 3, 3, 1.0)])
    return T, C, np.array(CYCLE3_START)


def cycle3_priors(y):
    """(nu, zeta) whose weight, a million times the data's, puts every draw
    on CYCLE3_TARGET to five digits"""
    zeta = np.full(3, 1e6 * float(np.sum(y)))
    return 1.0 + zeta * np.array(CYCLE3_TARGET), zeta


def ring(n):
    T, C = UC._fill(n, [(i, (i + 1) % n, 1, 1.0) for i in range(n)] + [(i, n, 2, 1.0) for i in range(n)])
    return T, C, np.array([1.0, 0.05])


def case(name, built):
    """the update_cases.Case of a builder's (T, C, truth), under the weak
    priors nu = 1 + 10 truth, zeta = 10 (``tight_priors`` gives the others)"""
    T, C, truth = built
    return UC.Case(name, T, C, 1.0 + 10.0 * truth, np.full(len(truth), 10.0), truth, (UC.ECS, UC.DCS))


def generator(built):
    """(S, s) at a builder's truth"""
    T, C, truth = built
    return UC.assemble(truth, T, C, True)


# (name, builder result) of the chains run bit for bit on the GPU, and of the accuracy cases on the CPU
def chain_structures():
    out = [(f"coxian{n}", coxian(n)) for n in COXIAN_N] + [(f"acyclic{n}", acyclic(n)) for n in ACYCLIC_N]
    out += [(f"symtied{n}{'c' if sc else ''}", symtied(n, sc)) for n in SYMTIED_N for sc in (False, True)]
    return out


# the weak-prior chains in which the warm start is both accepted and declined (60 sweeps, ECS, 30 % censored);
# seed 707 as the chains under the cases' own priors of test_gpu_update.py.  How often the refinement declines
# depends on the trajectory: over seeds 1, 2, 5, 123, 606, 707 it was 44 to 54 of 59 sweeps on coxian4, 58 on coxian8,
# 36 to 52 on symtied8, and 0 on symtied4 but for 2, 3 and 9 at seeds 2, 5 and 606
WARM_N, WARM_IT, WARM_SEED = 1500, 60, 707


def warm_structures():
    return [("coxian4", coxian(4)), ("coxian8", coxian(8)), ("symtied4", symtied(4)), ("symtied8", symtied(8))]
