"""CPU: the device specification (oracle "dev" variant, bit-exact with the HIP
kernels) samples the right conditional path law off BD-exit.

Every case of tests/pathlaw_ref.py's table through ``orc.dev_sweep``: the
bookkeeping invariants of every path, every (y, censoring) group's mean of z,
N and exits within 5 standard errors of the exact conditional expectations
(tests/estep_ref.py, completed by ``complete_stats``), and the censored
groups' time beyond y against the residual-life quantiles.  The truth helper
is anchored to mpmath, and the checker is shown to fail wrong truths and
doctored records.  tests/test_gpu_pathlaw.py runs the same cases on the GPU
kernels' own records; its printed worst z-scores equal this file's."""
import numpy as np
import pytest

import estep_ref as ER
import loglik_unif_ref as U
import pathlaw_ref as PL
from oracle.posterior import K_SIGMA
from phasetype_amd import complete_stats
from phasetype_amd.synth import bd_exit

_RECORDS = {}


@pytest.fixture
def spec_sweep(orc):
    """spec_sweep(case): the case's dev_sweep record (once per process for
    cases that differ only in a device setting), bridge modes reset after"""
    def run(case):
        S, s, (y, cen, _, _), _ = PL.inputs(case)
        k = (case["kind"], case["n"], case["method"], case["mhit"], case["probs"], case["cens"], case["key"],
             case["sweep"], case["bridge"])
        if k not in _RECORDS:
            orc.set_bridge(mhrs=case["bridge"] == "mhrs", dcs=case["bridge"] == "dcs")
            _RECORDS[k] = orc.dev_sweep(case["method"], S, s, y, cen, mhit=case["mhit"], key=case["key"],
                                        sweep=case["sweep"])
        return _RECORDS[k]
    yield run
    orc.set_bridge(False, False)


@pytest.mark.parametrize("name", [c["name"] for c in PL.CASES])
def test_spec_path_law(spec_sweep, name):
    case = PL.CASE_BY_NAME[name]
    S, s, lay, truths = PL.inputs(case)
    res = PL.check_record(spec_sweep(case), case, S, s, lay, truths)
    print(PL.report(case, res))
    assert not res["violations"], res["violations"]
    assert res["worst"] <= K_SIGMA, (name, np.round(res["z"]["z"], 2), np.round(res["z"]["N"], 2))
    assert res["resid"] <= 5.0, (name, res["resid"])


# ------------------------------------------------- anchor of the truth helper
ANCHORS = {"bd4": lambda: bd_exit(4), "cyclic3": lambda: U.CYCLIC, "acyclic8": lambda: PL.generator("acyclic", 8)}


@pytest.mark.parametrize("name", list(ANCHORS))
@pytest.mark.parametrize("cens", [0, 1])
def test_truth_against_mpmath(name, cens):
    """truth() == the 50-digit Van Loan reference completed the same way,
    within the E-step header's a-priori bound plus the relative 1e-12 that
    the completion's linear solve adds"""
    S, s = ANCHORS[name]()
    n = S.shape[0]
    yv = float(PL.ygrid(S, s, (0.5, 0.99))[cens])
    y, c = np.array([yv]), np.array([cens], np.int32)
    Z, N = PL.truth(S, s, yv, cens)
    m = ER.mp_reference(S, s, y, c)
    Zm, Nm, Em = complete_stats(S, s, m["Z"], m["N"], m["E"], m["A"])
    Nm = Nm + np.diag(Em)
    r = ER.estep(S, s, y, c)
    b = ER.bounds(n, y, c, r["klo"], r["khi"], np.ones(1, bool), r["yscale"])
    # the completion is linear in (Z, N, E, A): A's error passes through (-S)^-1 and the rates
    after = np.abs(np.linalg.inv(-S)).sum(1).max() * b["A"] * n
    rate = np.abs(S).max()
    tolZ = b["Z"] + after + 1e-12 * np.abs(Zm)
    tolN = max(b["N"], b["E"]) + after * rate + 1e-12 * np.abs(Nm)
    print(f"truth {name} cens {cens}: y {yv:.4g}, largest error {max(np.abs(Z - Zm).max(), np.abs(N - Nm).max()):.2e}, "
          f"tolerance {min(tolZ.min(), tolN.min()):.2e}")
    assert np.all(np.abs(Z - Zm) <= tolZ), (Z, Zm)
    assert np.all(np.abs(N - Nm) <= tolN), (N, Nm)
    assert abs(np.trace(N) - 1.0) <= n * tolN.max()  # one absorption per completed path
    if not cens:
        assert abs(Z.sum() - yv) <= n * b["Z"]


# --------------------------------------------------------- the checker's teeth
def test_checker_rejects_a_wrong_generator(spec_sweep):
    """the reversible-5 ECS records against the truth of a generator with one
    off-diagonal rate raised by 10 %: some cell beyond 5 standard errors"""
    case = PL.CASE_BY_NAME["ecs-reversible5"]
    S, s, lay, truths = PL.inputs(case)
    rec = spec_sweep(case)
    S2 = S.copy()
    S2[1, 2] *= 1.1
    S2[1, 1] -= S2[1, 2] - S[1, 2]
    wrong = PL.case_truths(S2, s, lay[3], case["method"])
    good = PL.group_zscores(rec["zq"], rec["zexp"], rec["N"], lay[2], truths, S)
    zs = PL.group_zscores(rec["zq"], rec["zexp"], rec["N"], lay[2], wrong, S2)
    print(f"right truth {good['worst']:.2f}, rate +10 %: {zs['worst']:.2f}")
    assert good["worst"] <= K_SIGMA < zs["worst"]


def test_checker_rejects_a_wrong_residual_life(orc):
    """The residual life given 1.2 y instead of y fails.  Shown on bd_exit(10)
    at its median with 16000 censored ECS paths: there the hazard still rises
    with the time survived, and the counts move by 9.0 sd (1.4 sd given y;
    the table's 4000 paths of that group see 4.1).  On the table's dense and
    cyclic generators the state at the median is already quasi-stationary,
    the residual life memoryless, and the two quantiles agree to the count:
    the residual-life check guards the law beyond y, not the time y itself
    (the cells of z and N do that)."""
    S, s = bd_exit(10)
    yv = float(PL.ygrid(S, s, (0.5,))[0])
    R = 16000
    rec = orc.dev_sweep(PL.ECS, S, s, np.full(R, yv), np.ones(R, np.int32), key=(0x5701, 0x71), sweep=1)
    assert not rec["flags"].any()
    tot = np.ldexp(rec["zq"].sum(1).astype(np.float64), -int(rec["zexp"]))
    right = np.abs(PL.residual_life(tot, yv, S, s)).max()
    wrong = np.abs(PL.residual_life(tot, yv, S, s, given=1.2 * yv)).max()
    print(f"residual life: given y {right:.2f} sd, given 1.2 y {wrong:.2f} sd")
    assert right <= 5.0 < wrong


def _doctored(rec):
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in rec.items()}
    out["N"] = np.ascontiguousarray(out["N"])
    return out


def test_checker_reports_doctored_records(spec_sweep):
    """acyclic 8 (forbidden cells below the diagonal): one count moved to a
    forbidden cell, one diagonal entry duplicated, one pre changed, one zq of
    an unvisited state set to 1: each is reported, with the observation"""
    case = PL.CASE_BY_NAME["ecs-acyclic8"]
    S, s, (y, cen, _, _), _ = PL.inputs(case)
    rec = spec_sweep(case)
    n = S.shape[0]
    assert PL.invariants(rec, S, y, cen, case["method"], s) == []
    N = rec["N"]
    exits = N.sum(2)
    # an observation with a jump 0 -> j, and one that never visited the last state
    i = int(np.nonzero(N[:, 0, 1:].sum(1) > 0)[0][3])
    j = 1 + int(np.argmax(N[i, 0, 1:] > 0))
    u = int(np.nonzero(exits[:, n - 1] == 0)[0][5])

    d = _doctored(rec)
    d["N"][i, 0, j] -= 1
    d["N"][i, j, 0] += 1  # S[j, 0] = 0: below the diagonal
    assert S[j, 0] == 0
    got = PL.invariants(d, S, y, cen, case["method"], s)
    assert any(v.startswith("count where the rate is 0") and f"[{i}]" in v for v in got), got
    assert any(v.startswith("flow") for v in got), got

    d = _doctored(rec)
    p = int(rec["pre"][i])
    d["N"][i, (p + 1) % n, (p + 1) % n] += 1
    got = PL.invariants(d, S, y, cen, case["method"], s)
    assert any(v.startswith("absorption") and f"[{i}]" in v for v in got), got

    d = _doctored(rec)
    d["pre"][i] = (p + 1) % n
    got = PL.invariants(d, S, y, cen, case["method"], s)
    assert got == [f"pre is not the exit state: obs [{i}]"], got

    d = _doctored(rec)
    d["zq"][u, n - 1] = 1
    got = PL.invariants(d, S, y, cen, case["method"], s)
    assert any(v.startswith("time in a state the path never left") and f"[{u}]" in v for v in got), got
