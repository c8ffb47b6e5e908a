"""CPU: the log-likelihood specification (include/pht_loglik.h) through the
host entry points and the tests' restatement (tests/loglik_spec.c); no GPU.

* pht_loglik_build + restatement against mpmath.expm at 50 digits, within
  64 * 2^-52 * cond2(Q) + 1e-13 * |l| (Q from numpy.linalg.eig(S)): the
  spectral sum loses cond(Q) ulps, the lmax y shift a few ulps of |l|.
* The contract off BD-exit (tests/evaluator_cases.py: the structures, stiff
  rates, Erlang, shared-rate Coxian, nearly equal rates, hypoexponential, at
  y from 1e-9 to 60): every value the evaluator returns is within
  E(A, l) = G 2^-52 A + 1e-13 |l| + ulp(l) of mpmath, everything else is a
  flagged draw or a counted bad observation; the guard rejects what it must
  and nothing of the well-conditioned list.
* Complex spectra and non-finite generators are flagged, never evaluated.
* The fixed-point totals are exact integer sums: within N * 2^-33 of
  math.fsum, identical under permutation.
* pht_theta_to_S against a numpy construction; log_lik's TT numbering is
  phtMCMC2's.
"""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import evaluator_cases as EC  # noqa: E402
import loglik_ref as R  # noqa: E402
import phasetype_amd as P  # noqa: E402
from phasetype_amd.synth import bd_exit, simulate_ph  # noqa: E402

Y_EDGE = [1e-9, 1e-3, 1000.0, 3000.0]


def _inputs(n):
    S, s = bd_exit(n)
    y, cens = simulate_ph(S, s, 60, seed=1, censor_frac=0.3)
    y = np.concatenate([y, Y_EDGE, Y_EDGE])
    cens = np.concatenate([cens, np.zeros(4, np.int32), np.ones(4, np.int32)]).astype(np.int32)
    return S, s, y, cens


def _truth(S, s, y, cens):
    import mpmath as mp

    n = S.shape[0]
    out = []
    with mp.workdps(50):
        Sm = mp.matrix(S.tolist())
        sv = mp.matrix(s.tolist())
        one = mp.matrix([1.0] * n)
        cache = {}
        for yi, ci in zip(y, cens):
            if yi not in cache:
                cache[yi] = mp.expm(Sm * mp.mpf(float(yi)))
            E = cache[yi]
            v = sv if ci == 0 else one
            out.append(mp.log(sum(E[0, j] * v[j] for j in range(n))))
    return out


@pytest.mark.parametrize("n", [3, 5, 10, 15, 20])
def test_block_and_restatement_against_mpmath(lib, n):
    import mpmath as mp

    S, s, y, cens = _inputs(n)
    blk = P.loglik_block(S, s)
    assert blk[:8].view(np.uint64)[0] == 0
    l = R.pointwise(blk[None, :], y, cens)[0]
    assert np.all(np.isfinite(l)), "no observation of these inputs is bad"
    truth = _truth(S, s, y, cens)
    cond = np.linalg.cond(np.linalg.eig(S)[1], 2)
    worst = 0.0
    for li, ti in zip(l, truth):
        err = float(abs(mp.mpf(float(li)) - ti))
        bound = 64 * 2.0 ** -52 * cond + 1e-13 * abs(float(ti))
        worst = max(worst, err / bound)
        assert err <= bound, (n, li, float(ti), err, bound)
    print(f"n={n}: cond2(Q)={cond:.3g}, worst error / bound = {worst:.3g}")
    # the contract's bound holds here too, and its ratio is measured: PHT_LL_G is 4 times the worst
    A = EC.spectral_A(blk, y, cens)
    ratio = 0.0
    for li, ti, Ai in zip(l, truth, A):
        err = float(abs(mp.mpf(float(li)) - ti))
        assert err <= EC.spectral_bound(Ai, ti), (n, li, float(ti), err, Ai)
        ratio = max(ratio, (err - 1e-13 * abs(float(ti)) - EC.ulp(ti)) / (2.0 ** -52 * Ai))
    print(f"n={n}: worst (error - 1e-13 |l| - ulp) / (2^-52 A) = {ratio:.3g}, worst 2^-52 A = {2.0 ** -52 * A.max():.3g}")


_CONTRACT = {}


def _contract(case):
    """One case through loglik_block, the restatement and the truth: dict(flag,
    y, cens, l, A, err, bound, tot); the contract is asserted here, once per
    case (the must lists below read the same record)."""
    import mpmath as mp

    key = EC.case_id(case)
    if key in _CONTRACT:
        return _CONTRACT[key]
    family, n, kw = case
    S, s = EC.generator(family, n, **kw)
    y, cens = EC.observations(S)
    blk = P.loglik_block(S, s)
    flag = int(blk[:8].view(np.uint64)[0])
    l = R.pointwise(blk[None, :], y, cens)[0]
    tot = R.totals(l[None, :])[0]
    rec = dict(flag=flag, y=y, cens=cens, l=l, tot=tot, A=np.full(len(y), np.nan), err=np.full(len(y), np.nan),
               bound=np.full(len(y), np.nan))
    if flag:
        assert np.all(np.isnan(l)), (key, "a flagged draw is never evaluated")
    else:
        truth = EC.truths(S, s, y, cens)
        rec["A"] = EC.spectral_A(blk, y, cens)
        for k in np.flatnonzero(np.isfinite(l)):
            rec["err"][k] = float(abs(mp.mpf(float(l[k])) - truth[k]))
            rec["bound"][k] = EC.spectral_bound(rec["A"][k], truth[k])
        # a rejected pair is reported: NaN pointwise and counted
        assert tot[2] == np.sum(np.isnan(l)) and tot[3] == np.sum(np.isfinite(l)), (key, tot)
        assert not np.any(np.isinf(l)), key
    fin = np.isfinite(l)
    ratio = (np.max((rec["err"][fin] - 1e-13 * np.abs(l[fin]) - np.spacing(np.abs(l[fin])))
                    / (2.0 ** -52 * rec["A"][fin])) if fin.any() else float("nan"))
    rec["ratio"] = ratio
    print(f"{key}: flag {flag}, accepted {int(fin.sum())} of {len(y)}, worst error "
          f"{np.max(rec['err'][fin]) if fin.any() else float('nan'):.3g}, worst error / bound "
          f"{np.max(rec['err'][fin] / rec['bound'][fin]) if fin.any() else float('nan'):.3g}, "
          f"worst 2^-52 A accepted {2.0 ** -52 * np.max(rec['A'][fin]) if fin.any() else float('nan'):.3g}, "
          f"worst (error - 1e-13 |l| - ulp) / (2^-52 A) {ratio:.3g}")
    _CONTRACT[key] = rec
    for k in np.flatnonzero(fin):
        assert rec["err"][k] <= rec["bound"][k], (key, y[k], cens[k], l[k], rec["err"][k], rec["bound"][k])
    return rec


def test_header_constants_are_the_tests():
    import re

    with open(os.path.join(os.path.dirname(HERE), "include", "pht_loglik.h")) as f:
        h = f.read()
    assert float(re.search(r"#define PHT_LL_G ([0-9.]+)", h).group(1)) == EC.G
    assert float.fromhex(re.search(r"#define PHT_LL_EMAX (\S+)", h).group(1)) == EC.E_MAX <= 1e-6
    assert re.search(r"#define PHT_LL_F_ILLCOND 16u", h) and P.LL_F_ILLCOND == 16


@pytest.mark.parametrize("case", EC.CASES, ids=EC.case_id)
def test_spectral_contract_off_bd_exit(lib, case):
    """loglik_block, then the restatement, against the truth: every finite
    value within E(A, l) (A recomputed in numpy from the block), every other
    pair a flagged draw or a NaN counted in nbad.  PHT_LL_G is 4 times the
    worst (error - 1e-13 |l| - ulp(l)) / (2^-52 A) this test and
    test_block_and_restatement_against_mpmath print over the accepted pairs:
    90.1, at bd_exit(20), y = 13.0, exact."""
    _contract(case)


def test_guard_accepts_the_well_conditioned_list(lib):
    """The guard may not hide failures.  No draw of bd_exit(n) at this file's
    inputs, nor of acyclic, reversible and stiff at n = 6 and 12 with
    y >= 1e-3, is flagged, and none of their observations is bad.

    PHT_LL_EMAX is the largest power of two below 1e-6.  With 16 times the
    measured A the list would still be accepted in full, except bd_exit(20):
    its 2^-52 A reaches 7.8e-10 (y = 1e-9, exact; 6.6e-10 at y = 0.08), which
    G = 361 leaves 3.4 times below the guard, and no power of two below 1e-6
    leaves 16.  That headroom is printed, the 16 asserted for the rest."""
    worst = {}
    for n in (3, 5, 10, 15, 20):
        S, s, y, cens = _inputs(n)
        blk = P.loglik_block(S, s)
        assert blk[:8].view(np.uint64)[0] == 0
        assert np.all(np.isfinite(R.pointwise(blk[None, :], y, cens)[0]))
        worst[f"bd-{n}"] = float(np.max(EC.spectral_A(blk, y, cens)))
    for family in ("acyclic", "reversible", "stiff"):
        for n in EC.STRUCT_N:
            rec = _contract((family, n, {}))
            keep = rec["y"] >= 1e-3
            assert rec["flag"] == 0 and np.all(np.isfinite(rec["l"][keep])), (family, n)
            worst[f"{family}-{n}"] = float(np.max(rec["A"][keep]))
    for key, A in worst.items():
        room = EC.E_MAX / (EC.G * 2.0 ** -52 * A)
        print(f"{key}: worst 2^-52 A = {2.0 ** -52 * A:.3g}, {room:.3g} times below the guard")
        assert room >= (16.0 if key != "bd-20" else 1.0), (key, room)


def test_guard_rejects_the_ill_conditioned_list(lib):
    """Erlang and the shared-rate Coxian (exactly defective) are flagged
    ILLCOND at every n; with nearly equal rates (n = 6, 10, every eps) and at
    hypoexp(3), y = 1e-9 (f = 6e-18 from coefficients of order one) every
    observation is rejected or within the bound.  The rows that were finite
    and wrong by tens of nats (gapped n = 6, eps = 1e-3; n = 10, eps = 1e-9)
    are rejected."""
    for family in ("erlang", "coxian_shared"):
        for n in EC.NEW_N:
            rec = _contract((family, n, {}))
            assert rec["flag"] & P.LL_F_ILLCOND and not rec["flag"] & P.LL_F_NONFINITE, (family, n, rec["flag"])
    for n in (6, 10):
        for eps in EC.EPS:
            rec = _contract(("gapped", n, {"eps": eps}))  # (asserts the bound on whatever is finite)
            assert rec["flag"] or rec["tot"][2] + rec["tot"][3] == len(rec["y"])
    for n, eps in ((6, 1e-3), (10, 1e-9)):
        assert _contract(("gapped", n, {"eps": eps}))["flag"] & P.LL_F_ILLCOND
    rec = _contract(("hypoexp", 3, {}))
    k = np.flatnonzero((rec["y"] == 1e-9) & (rec["cens"] == 0))[0]
    assert rec["flag"] == 0 and (np.isnan(rec["l"][k]) or rec["err"][k] <= rec["bound"][k])
    assert rec["tot"][2] >= 1, "at HEAD this value was finite with nothing behind it"


def test_erlang_closed_forms_guard_the_truth():
    """The expm truth against log f = n log lam + (n - 1) log y - lam y -
    log (n - 1)! and the Poisson-sum survival, to 1e-25 relative."""
    for n in EC.NEW_N:
        S, s = EC.erlang(n)
        y, cens = EC.observations(S)
        for yi, ci in zip(y, cens):
            t, c = EC.truth(S, s, float(yi), int(ci)), EC.erlang_closed(n, EC.LAM, float(yi), int(ci))
            assert abs(t - c) <= 1e-25 * abs(c), (n, yi, ci, t, c)


def test_far_tail_is_finite(lib):
    """The shift by lmax: bd_exit(3) at y = 3000 is -3500.305, where the
    unshifted sum underflows to log 0."""
    S, s = bd_exit(3)
    l = R.pointwise(P.loglik_block(S, s)[None, :], np.array([3000.0]), np.zeros(1, np.int32))[0, 0]
    assert abs(l - (-3500.305)) < 1e-3


def test_unusable_draws_are_flagged(lib):
    cyc = np.array([[-1.1, 1, 0], [0, -1.1, 1], [1, 0, -1.1]])
    n = 3
    out = np.zeros(P.load().pht_loglik_bytes(n), np.uint8)
    rc = lib.pht_loglik_build(n, np.ascontiguousarray(cyc.reshape(-1, order="F")), 0.1 * np.ones(3),
                              out.ctypes.data, len(out))
    assert rc > 0 and out[:8].view(np.uint64)[0] == rc
    S, s = bd_exit(3)
    S[1, 0] = np.nan
    rc = lib.pht_loglik_build(n, np.ascontiguousarray(S.reshape(-1, order="F")), s, out.ctypes.data, len(out))
    assert rc > 0 and out[:8].view(np.uint64)[0] == rc
    # the restatement never evaluates a flagged block
    assert np.all(np.isnan(R.pointwise(out[None, :], np.array([1.0, 2.0]), np.zeros(2, np.int32))))
    assert np.isnan(P.loglik_total([0], [0], [0], [True])[0])
    assert P.loglik_total([-3], [1 << 31], [1], [False])[0] == -np.inf


def test_build_rejects_bad_arguments(lib):
    out = np.zeros(8, np.uint8)
    S, s = bd_exit(3)
    assert lib.pht_loglik_build(3, np.ascontiguousarray(S.reshape(-1)), s, out.ctypes.data, len(out)) < 0
    assert lib.pht_loglik_bytes(33) < 0 and lib.pht_loglik_bytes(0) < 0
    assert lib.pht_loglik_bytes(20) == 8 * 62


@pytest.mark.parametrize("n", [5, 10])
def test_fixed_point_totals(lib, n):
    S, s = bd_exit(n)
    y, cens = simulate_ph(S, s, 500, seed=2, censor_frac=0.3)
    blk = P.loglik_block(S, s)[None, :]
    l = R.pointwise(blk, y, cens)
    tot = R.totals(l)[0]
    N = len(y)
    assert tot[2] == 0 and tot[3] == N
    val = P.loglik_total(tot[0:1], tot[1:2], tot[2:3], [False])[0]
    assert abs(val - math.fsum(l[0])) <= N * 2.0 ** -33
    perm = np.random.default_rng(3).permutation(N)
    tot_p = R.totals(R.pointwise(blk, y[perm], cens[perm]))[0]
    assert np.array_equal(tot, tot_p)
    # two shards add to the whole
    a, b = R.totals(l[:, :123])[0], R.totals(l[:, 123:])[0]
    assert np.array_equal(a + b, tot)


def test_fixed_point_bad_observation(lib):
    """NaN (bad) observations are counted, not summed."""
    tot = R.totals(np.array([[1.25, np.nan, -2.5]]))[0]
    assert tot.tolist() == [-1, -(1 << 30), 1, 2]  # 1.25 = 1 + 2^30 2^-32; -2.5 = -2 - 2^31 2^-32 (ties to even)
    assert tot[0] + tot[1] * 2.0 ** -32 == -1.25


def test_waic_recurrence_against_numpy(lib):
    from scipy.special import logsumexp

    Ss, ss = R.scaled_draws(5)
    S, s = bd_exit(5)
    y, cens = simulate_ph(S, s, 200, seed=4, censor_frac=0.3)
    blocks = np.stack([P.loglik_block(a, b) for a, b in zip(Ss, ss)])
    l = R.pointwise(blocks, y, cens)
    st = R.waic_state(l)
    assert np.all(st["cnt"] == 5)
    # batching the draws does not change the state
    st2 = R.waic_state(l[3:], R.waic_state(l[:3]))
    for k in st:
        assert np.array_equal(st[k], st2[k]), k
    w = P.waic_from_state(st)
    lppd_i = logsumexp(l, axis=0) - np.log(5)
    p_i = np.var(l, axis=0, ddof=1)
    assert np.all(np.abs(w["pointwise"][0] - lppd_i) <= 1e-12 * np.maximum(1, np.abs(lppd_i)))
    assert np.all(np.abs(w["pointwise"][1] - p_i) <= 1e-12 * np.maximum(1, np.abs(p_i)))
    assert abs(w["waic"] + 2 * (lppd_i.sum() - p_i.sum())) <= 1e-10 * abs(w["waic"])


def test_theta_to_S_matches_numpy(lib):
    rng = np.random.default_rng(5)
    n = 4
    T = np.zeros((n + 1, n + 1), np.int32)
    T[0, 1], T[0, 2], T[1, 0], T[1, 4], T[2, 3], T[2, 4], T[3, 0], T[3, 4], T[0, 4] = 1, 2, 3, 4, 1, 5, 2, 6, 6
    Cm = np.ones((n + 1, n + 1))
    Cm[2, 3], Cm[3, 0] = 2.5, 0.75
    theta = rng.gamma(2.0, 1.0, 6)
    S, s = P.theta_to_S(theta, T, Cm)
    G = np.where(T > 0, theta[np.maximum(T, 1) - 1] * Cm, 0.0)
    Sn = G[:n, :n].copy()
    sn = G[:n, n].copy()
    for i in range(n):
        Sn[i, i] = -G[i].sum()
    assert np.all(np.abs(S - Sn) <= np.spacing(np.abs(Sn)))
    assert np.array_equal(s, sn)


def test_tt_names_numbered_as_phtMCMC2(lib):
    """log_lik numbers a matrix of names the way phtMCMC2 does (sorted names
    without "0", "C" or "en_US" collation), so its columns are the chain's."""
    TT = np.array([["0", "b", "S12", "a"], ["s1", "0", "0", "b"], ["0", "S12", "0", "Z"], ["0", "0", "0", "0"]],
                  dtype=object)
    for coll in ("C", "en_US"):
        names = [v for v in P._r_sort(set(TT.reshape(-1).tolist()), coll) if v != "0"]
        T, got = P._tt_numbers(TT, coll)
        assert got == names
        for i in range(4):
            for j in range(4):
                assert T[i, j] == (["0"] + names).index(TT[i, j])
    Ti, none = P._tt_numbers(np.array([[0, 1], [0, 0]]))
    assert none is None and Ti.dtype == np.int32
    # the chain's columns must match the generator's variables
    with pytest.raises(ValueError):
        P._chain_blocks(np.ones((2, 3)), TT, None, None)
    with pytest.raises(ValueError):
        P._chain_blocks(dict(samples=np.ones((2, 5)), TT=TT, vars=["x"] * 5), None, None, None)
