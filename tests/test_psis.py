"""CPU: the PSIS-LOO specification (include/pht_psis.h) through the tests'
restatement (tests/psis_spec.c); no GPU.

* The restatement against the published algorithm written here with
  np.log1p, np.expm1 and scipy's logsumexp, within 1e-9 (the two sides differ
  by rounding only, about S 2^-53; a tail length or cutoff off by one moves
  khat by more than 1e-3).
* Validity: an exponential model with one outlier, against the exact
  leave-one-out density.
* Edge cases: short chains, constant tails, ties at the cutoff, NaN, flagged
  draws, the tail-length table.
* loo_from_psis / loo_compare arithmetic.
"""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import psis_ref as R  # noqa: E402


# ------------------------------------------- the published algorithm in numpy
def np_gpdfit(x):
    """Zhang & Stephens (2009) as gpdfit of the loo package; x ascending."""
    M = len(x)
    G = 30 + int(math.floor(math.sqrt(M)))
    j = np.arange(1, G + 1)
    xs = x[int(math.floor(M / 4 + 0.5)) - 1]
    theta = 1.0 / x[-1] + (1.0 - np.sqrt(G / (j - 0.5))) / 3.0 / xs
    k = np.mean(np.log1p(-theta[:, None] * x[None, :]), axis=1)
    L = M * (np.log(-theta / k) - k - 1.0)
    w = 1.0 / np.sum(np.exp(L[None, :] - L[:, None]), axis=1)
    th = float(np.sum(theta * w))
    k = float(np.mean(np.log1p(-th * x)))
    sigma = -k / th
    return (k * M + 5.0) / (M + 10.0), sigma


def np_psis(l):
    from scipy.special import logsumexp

    S, N = l.shape
    elpd, khat, lppd = np.zeros(N), np.full(N, np.inf), np.zeros(N)
    M = min(S // 5, int(math.ceil(3.0 * math.sqrt(S))))
    for i in range(N):
        li = l[:, i]
        lw = -li - np.max(-li)
        if M >= 5:
            order = np.argsort(lw, kind="stable")
            tail, c = order[S - M:], lw[order[S - M - 1]]
            x = np.exp(lw[tail]) - np.exp(c)
            if x[-1] != x[0]:
                with np.errstate(all="ignore"):
                    k, sigma = np_gpdfit(x)
                if np.isfinite(k) and np.isfinite(sigma) and sigma > 0:
                    p = (np.arange(1, M + 1) - 0.5) / M
                    q = sigma * np.expm1(-k * np.log1p(-p)) / k if k != 0 else -sigma * np.log1p(-p)
                    lw = lw.copy()
                    lw[tail] = np.log(q + np.exp(c))
                    lw = np.minimum(lw, 0.0)
                    khat[i] = k
        elpd[i] = logsumexp(lw + li) - logsumexp(lw)
        lppd[i] = logsumexp(li) - math.log(S)
    return elpd, khat, lppd


@pytest.mark.parametrize("S", [25, 64, 65, 400, 1000, 4096])
def test_restatement_against_numpy(S):
    rng = np.random.default_rng(100 + S)
    N = 24
    # columns of different spread: light and heavy tails of the ratios
    l = -2.0 + rng.normal(size=(S, N)) * np.linspace(0.1, 1.5, N)[None, :] - rng.exponential(0.3, size=(S, N))
    r = R.psis(l)
    elpd, khat, lppd = np_psis(l)
    assert np.all(r["flags"] == 0)
    d = [float(np.max(np.abs(r["elpd_i"] - elpd))), float(np.max(np.abs(r["khat"] - khat))),
         float(np.max(np.abs(r["lppd_i"] - lppd)))]
    print(f"S = {S}: largest |difference| elpd {d[0]:.3g} khat {d[1]:.3g} lppd {d[2]:.3g}")
    assert max(d) <= 1e-9, d


# --------------------------------------------------- exact leave-one-out
def test_validity_against_exact_loo(lib):
    import loglik_ref as LR
    import phasetype_amd as P

    N, S = 200, 4000
    rng = np.random.default_rng(2024)
    y = rng.exponential(1.0, N)
    y[0] = 12.0
    lam = rng.gamma(1.0 + N, 1.0 / (1.0 + y.sum()), S)  # the exact posterior under the Gamma(1, 1) prior
    blocks = np.stack([P.loglik_block(np.array([[-v]]), np.array([v])) for v in lam])
    l = LR.pointwise(blocks, y, np.zeros(N, np.int32))
    r = R.psis(l)
    a, b = float(N), 1.0 + y.sum() - y
    exact = math.log(a) + a * np.log(b) - (a + 1.0) * np.log(b + y)
    err = np.abs(r["elpd_i"] - exact)
    print(f"max |elpd - exact| {err.max():.4f} at {int(np.argmax(err))}; khat[0] {r['khat'][0]:.3f}; "
          f"|lppd_0 - exact_0| {abs(r['lppd_i'][0] - exact[0]):.4f}; |elpd_0 - exact_0| {err[0]:.4f}")
    assert err.max() <= 0.05
    assert int(np.argmax(r["khat"])) == 0
    assert err[0] < 0.25 * abs(r["lppd_i"][0] - exact[0])


# ------------------------------------------------------------- edge cases
def _plain_is(l):
    from scipy.special import logsumexp

    return math.log(l.shape[0]) - logsumexp(-l, axis=0)


def test_short_chain_is_plain_importance_sampling():
    rng = np.random.default_rng(5)
    l = rng.normal(-1.0, 0.5, (24, 7))
    r = R.psis(l)
    assert np.all(r["flags"] == R.F_SHORT) and np.all(np.isposinf(r["khat"]))
    assert np.max(np.abs(r["elpd_i"] - _plain_is(l))) <= 1e-12
    assert np.all(R.psis(l[:1])["flags"] == R.F_SHORT)


def test_identical_draws_constant_tail():
    l = np.tile(np.array([[-1.25, -3.0, -0.5]]), (100, 1))
    r = R.psis(l)
    assert np.all(r["flags"] == R.F_CONST) and np.all(np.isposinf(r["khat"]))
    assert np.max(np.abs(r["elpd_i"] - l[0])) <= 1e-12
    assert np.max(np.abs(r["lppd_i"] - l[0])) <= 1e-12


def test_ties_at_the_cutoff():
    rng = np.random.default_rng(6)
    S = 100  # M = 20
    base = rng.normal(-2.0, 0.8, (S, 4))
    # many copies of the value at the cutoff, inside and outside the tail
    for i in range(4):
        order = np.argsort(base[:, i])  # ascending l: the first are the largest ratios
        base[order[15:15 + 4 * (i + 1)], i] = base[order[20], i]
    r = R.psis(base)
    # a permutation of the draws among the ties: the same outputs, bit for bit
    cols = []
    for i in range(4):
        tied = np.flatnonzero(base[:, i] == base[np.argsort(base[:, i])[20], i])
        assert len(tied) >= 5
        perm = np.arange(S)
        perm[tied] = tied[::-1]
        cols.append(base[perm, i])
    r2 = R.psis(np.column_stack(cols))
    for k in ("elpd_i", "khat", "lppd_i"):
        assert np.array_equal(r[k].view(np.uint64), r2[k].view(np.uint64)), k
    for i in range(4):
        assert r["flags"][i] in (0, R.F_FIT)
        assert np.isfinite(r["khat"][i]) == (r["flags"][i] == 0)
        assert np.isfinite(r["elpd_i"][i])
    # distinct l that collide in lw: which of them enters the tail is open, the outputs are not
    l = rng.normal(-2.0, 0.8, S)
    l[np.argmin(l)] = -40.0  # mx = 40: weights near -38 have a coarser grid than l near -2
    o = np.argsort(l)
    l[o[20]] = np.nextafter(l[o[19]], np.inf)
    lw = -l - np.max(-l)
    assert lw[o[20]] == lw[o[19]] and l[o[20]] != l[o[19]]
    ra = R.psis(l[:, None])
    l2 = l.copy()
    l2[[o[19], o[20]]] = l2[[o[20], o[19]]]
    rb = R.psis(l2[:, None])
    for k in ("elpd_i", "khat", "lppd_i"):
        if k != "lppd_i":  # lppd sums the l themselves, in draw order
            assert np.array_equal(ra[k].view(np.uint64), rb[k].view(np.uint64)), k


def test_nan_and_flagged_draws():
    rng = np.random.default_rng(7)
    l = rng.normal(-1.0, 0.5, (60, 5))
    l[17, 2] = np.nan
    r = R.psis(l)
    assert r["flags"][2] == R.F_BAD and all(np.isnan(r[k][2]) for k in ("elpd_i", "khat", "lppd_i"))
    assert np.all(r["flags"][[0, 1, 3, 4]] == 0)
    usable = np.ones(60, bool)
    usable[[3, 17, 40]] = False
    l[3] = np.nan  # a flagged draw's row is NaN and never read
    r2 = R.psis(l, usable)
    assert r2["n_draws_used"] == 57 and np.all(r2["flags"] == 0)
    ref = R.psis(l[usable])
    assert np.array_equal(r2["elpd_i"], ref["elpd_i"])


def test_tail_length_table():
    for S in range(25, 16385):
        m = math.isqrt(9 * S - 1) + 1
        assert m * m >= 9 * S > (m - 1) * (m - 1)
        assert R.tail_len(S) == min(S // 5, m), S
    assert R.tail_len(24) == 4 and R.tail_len(25) == 5 and R.tail_len(16384) == 384
    assert R.spec().spec_grid(384) == 49 and R.spec().spec_grid(5) == 32


def test_log1p_expm1_forms():
    for z in (-0.9, -1e-3, -1e-17, 0.0, 1e-17, 1e-9, 0.3, 5.0):
        assert abs(R.spec().spec_log1p(z) - math.log1p(z)) <= 4e-16 * max(abs(math.log1p(z)), 1e-300)
        assert abs(R.spec().spec_expm1(z) - math.expm1(z)) <= 4e-16 * max(abs(math.expm1(z)), 1e-300)
    assert R.spec().spec_expm1(-800.0) == -1.0


def test_loo_and_compare_arithmetic():
    import phasetype_amd as P

    r = dict(elpd_i=np.array([-1.0, -2.0, -4.0]), lppd_i=np.array([-0.5, -1.5, -3.0]),
             khat=np.array([0.1, 0.69, 0.8]), n_draws_used=1000)
    r["p_loo_i"] = r["lppd_i"] - r["elpd_i"]
    a = P.loo_from_psis(r)
    assert a["elpd_loo"] == -7.0 and a["p_loo"] == 2.0 and a["looic"] == 14.0 and a["lppd"] == -5.0
    assert a["se_elpd_loo"] == pytest.approx(math.sqrt(3 * np.var([-1.0, -2.0, -4.0])))
    assert a["khat_threshold"] == pytest.approx(1.0 - 1.0 / 3.0) and a["n_khat_above"] == 2
    assert a["n_draws_used"] == 1000
    r["n_draws_used"] = 100000
    assert P.loo_from_psis(r)["khat_threshold"] == 0.7 and P.loo_from_psis(r)["n_khat_above"] == 1
    b = dict(pointwise=(np.array([-1.5, -1.0, -4.5]), None, None))
    c = P.loo_compare(a, b)
    assert c["elpd_diff"] == pytest.approx(0.0)
    assert c["se_diff"] == pytest.approx(math.sqrt(3 * np.var([0.5, -1.0, 0.5])))
    with pytest.raises(ValueError):
        P.loo_compare(a, dict(pointwise=(np.zeros(2), None, None)))
