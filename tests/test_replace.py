"""CPU: include/pht_replace.h through the tests' restatement
(tests/replace_spec.c) against mpmath truths, on the generators of
tests/evaluator_cases.py with ages = m (0.05 .. 3.2) and the cost pairs (1, 10)
and (1, 1.5): the restricted mean within the header's bound and the recorded
constants honest (largest ratio <= constant <= 4 x largest ratio); every
returned bracket around the true root; g(t^) against the truth's minimum; the
identity g = (cf - cp) h; every reachable flag path; the posterior summary and
the fleet add-on; the library's host function bit for bit the restatement.

stiff6 (mu m = 4.6e4): only the first age lies within mu tau <= 1400, the
horizon the specification inherits from pht_q_meta, so its outcome is EDGE and
NEVER from one good age, not an interior root; the other six ages are flagged
and counted.  PHT_RP_F_EVAL and PHT_RP_F_CAP need a bad evaluation strictly
inside a bracket of good ones, or 400 steps: no input here reaches them."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import replace_ref as R  # noqa: E402

MU_TAU = (1e-9, 1e-3, 1.0, 30.0, 1000.0)
CP = np.array([p[0] for p in R.PAIRS])
CF = np.array([p[1] for p in R.PAIRS])


def _mp(x):
    import mpmath as mp

    return mp.mpf(float(x))


@pytest.fixture(scope="module")
def cases():
    """per named generator: S, s, m, the grid, the restatement's result"""
    out = {}
    for name in R.NAMED:
        S, s = R.named(name)
        m = R.mean(S, s)
        ages = m * R.GRID
        out[name] = dict(S=S, s=s, n=S.shape[0], m=m, ages=ages, r=R.replace([S], [s], ages, CP, CF))
    return out


@pytest.fixture(scope="module")
def m_ratios():
    """|M^ - M| / (eps(k_hi) M) at mu tau of MU_TAU for every named generator"""
    rows = []
    for name in R.NAMED:
        S, s = R.named(name)
        n, mu = S.shape[0], float(np.max(-np.diag(S)))
        taus = np.array(MU_TAU) / mu
        ev = R.rmean(S, s, taus)
        for i, tau in enumerate(taus):
            assert not ev["bad"][i], (name, MU_TAU[i])
            tr = R.truth(S, s, tau)["M"]
            err = abs(_mp(ev["M"][i]) - tr)
            rows.append((name, MU_TAU[i], int(ev["khi"][i]), float(err), float(tr),
                         float(err / tr) / R.spec().rpspec_eps(n, int(ev["khi"][i])), n))
    return rows


def test_rmean_within_the_bound_and_the_constant_is_honest(m_ratios):
    worst = max(m_ratios, key=lambda r: r[5])
    print("largest |M^ - M| / (eps M):", worst)
    for name, lam, khi, err, M, ratio, n in m_ratios:
        assert err <= R.M_bound(n, khi, M), (name, lam, err, R.M_bound(n, khi, M))
        # a few 2^-53 for mu tau <= 1, about 55 x 2^-53 at mu tau = 30 (the series' own accuracy)
        assert err / M <= (8 if lam <= 1 else 110) * 2.0 ** -53 or lam > 30, (name, lam, err / M * 2.0 ** 53)
    M_R = R.spec().rpspec_M_R()
    assert worst[5] <= M_R <= 4 * worst[5], (worst[5], M_R)


def test_M_tends_to_tau_and_to_m(cases):
    for name, c in cases.items():
        mu = float(np.max(-np.diag(c["S"])))
        ev = R.rmean(c["S"], c["s"], np.array([1e-12 / mu, 1000.0 / mu]))
        assert abs(ev["M"][0] / (1e-12 / mu) - 1) < 1e-11, name
        assert ev["M"][1] <= c["m"] * (1 + 1e-12) and ev["M"][1] > 0, name


@pytest.fixture(scope="module")
def d_points(cases):
    """(name, pair, tau, D^, D_true, bound, kind) at the grid's good ages and
    at lo, hi, t^ of every refined root"""
    rows = []
    for name, c in cases.items():
        S, s, n, r = c["S"], c["s"], c["n"], c["r"]
        good = r["age_flags"][0] == 0
        pts = [(float(t), "age") for t in c["ages"][good]]
        for p in range(len(CP)):
            if r["flags"][0, p] == 0:
                pts += [(float(r["lo"][0, p]), f"lo{p}"), (float(r["hi"][0, p]), f"hi{p}"),
                        (float(r["t"][0, p]), f"t{p}")]
        ev = R.evaluate(S, s, [t for t, _ in pts], tmax=c["ages"][-1])
        for i, (tau, kind) in enumerate(pts):
            assert not ev["bad"][i]
            tr = R.truth(S, s, tau)
            for p in range(len(CP)):
                if kind != "age" and not kind.endswith(str(p)):
                    continue
                c0 = _mp(CP[p]) / (_mp(CF[p]) - _mp(CP[p]))
                Dt = tr["h"] * tr["M"] - tr["F"] - c0
                Dh = R.spec().rpspec_D(ev["lS"][i], ev["lf"][i], ev["M"][i], CP[p], CF[p])
                bound = R.D_bound(n, int(ev["khi"][i]), tr["h"] * tr["M"], tr["F"], c0)
                rows.append(dict(name=name, p=p, tau=tau, kind=kind[:-1] if kind != "age" else kind, Dh=Dh,
                                 Dt=float(Dt), err=float(abs(_mp(Dh) - Dt)), bound=bound, tr=tr,
                                 lS=ev["lS"][i], lf=ev["lf"][i], M=ev["M"][i], khi=int(ev["khi"][i])))
    return rows


def test_D_within_the_bound_and_the_constant_is_honest(d_points):
    D_R = R.spec().rpspec_D_R()
    ratios = [(r["err"] / (r["bound"] / D_R), r["name"], r["p"], r["kind"]) for r in d_points]
    worst = max(ratios)
    print("largest |D^ - D| / (eps (h M + F + c0)):", worst)
    for r in d_points:
        assert r["err"] <= r["bound"], (r["name"], r["p"], r["kind"], r["err"], r["bound"])
    assert worst[0] <= D_R <= 4 * worst[0], (worst[0], D_R)


def test_brackets_hold_the_true_root(cases, d_points):
    """D_true(lo) <= delta and D_true(hi) >= -delta, delta the header's bound;
    the stop rule holds; t^ lies inside"""
    seen = 0
    for r in d_points:
        if r["kind"] == "lo":
            assert r["Dt"] <= r["bound"], r
            seen += 1
        if r["kind"] == "hi":
            assert r["Dt"] >= -r["bound"], r
    for name, c in cases.items():
        res = c["r"]
        for p in range(len(CP)):
            if res["flags"][0, p] == 0:
                lo, hi, t = res["lo"][0, p], res["hi"][0, p], res["t"][0, p]
                assert lo <= t <= hi and hi - lo <= R.spec().rpspec_rtol() * hi, (name, p)
                assert res["nev"][0, p] <= 64 * 8 + 1, (name, p, res["nev"][0, p])
    assert seen == 10  # eight at (1, 10) without stiff6 plus gapped6, erlang6 and gapped6 at (1, 1.5)
    print("largest nev:", max(int(c["r"]["nev"].max()) for c in cases.values()))


def test_g_at_the_root_and_the_identity(cases, d_points):
    """g(t^) within the bound of g_true(tau*_true), tau*_true by findroot in
    the returned cell: the evaluation's error at t^ (M's bound, eps for lS
    through F, six roundings) plus the truth's own |g(t^) - g(tau*)| <=
    (cf - cp) Fbar / M^2 max|D| (hi - lo); and g = (cf - cp) h at t^ up to
    (cf - cp) |D| / M, |D| <= the cell's largest |D_true| plus D's bound"""
    by = {(r["name"], r["p"], r["kind"]): r for r in d_points if r["kind"] != "age"}
    seen = 0
    for name, c in cases.items():
        S, s, n, res = c["S"], c["s"], c["n"], c["r"]
        for p in range(len(CP)):
            if res["flags"][0, p] != 0:
                continue
            seen += 1
            lo, hi, th = by[name, p, "lo"], by[name, p, "hi"], by[name, p, "t"]
            cp, cf = _mp(CP[p]), _mp(CF[p])
            root = R.root_true(S, s, lo["tau"], hi["tau"], CP[p], CF[p])
            g_root = R.g_true(S, s, root, CP[p], CF[p], extra=40)
            w = _mp(hi["tau"]) - _mp(lo["tau"])
            assert _mp(lo["tau"]) - w <= root <= _mp(hi["tau"]) + w, (name, p, root)
            tr = th["tr"]
            eps = R.spec().rpspec_eps(n, th["khi"])
            g_t = (cp + (cf - cp) * tr["F"]) / tr["M"]
            rel = R.spec().rpspec_M_R() * eps + eps * float((cf - cp) * tr["Fbar"] / (cp + (cf - cp) * tr["F"])) \
                + 6 * 2.0 ** -53
            dmax = max(abs(lo["Dt"]), abs(hi["Dt"]))
            flat = float((cf - cp) * lo["tr"]["Fbar"] / lo["tr"]["M"] ** 2 * w) * dmax
            g_hat = float(res["g"][0, p])
            err = float(abs(_mp(g_hat) - g_root))
            tol = float(g_t) * rel + flat
            print(f"{name} pair {p}: t^/m {res['t'][0, p] / c['m']:.6f} g {g_hat:.15g} error {err:.3g} tol {tol:.3g}")
            assert err <= tol, (name, p, err, tol)
            # the identity, from the restatement's own values at t^
            h_hat = float(np.exp(th["lf"] - th["lS"]))
            resid = abs(g_hat - (CF[p] - CP[p]) * h_hat)
            itol = float((cf - cp) / tr["M"]) * (dmax + th["bound"]) + 8 * 2.0 ** -53 * g_hat
            assert resid <= itol, (name, p, resid, itol)
            print(f"   identity: |g - (cf - cp) h| / g = {resid / g_hat:.3g}")
    assert seen == 10


def test_outcomes_of_the_grid(cases):
    """the table of the issue: interior roots at (1, 10) with D signs - .. - + .. +,
    erlang6's interior root at (1, 1.5) near 1.40 m, EDGE and NEVER elsewhere"""
    for name, c in cases.items():
        r, ages, m = c["r"], c["ages"], c["m"]
        assert r["draw_flags"][0] == 0 and r["m"][0] == m
        if name == "stiff6":
            assert np.array_equal(r["age_flags"][0], [0] + [R.A_BEYOND] * 6)
            assert np.all(np.isnan(r["M"][0, 1:])) and np.isfinite(r["M"][0, 0])
            assert np.all(r["flags"][0] == (R.F_EDGE | R.F_NEVER)) and np.all(r["j"][0] == 0)
            continue
        assert not r["age_flags"][0].any()
        for p in range(2):
            D = np.array([R.spec().rpspec_D(r["lS"][0, i], r["lf"][0, i], r["M"][0, i], CP[p], CF[p])
                          for i in range(7)])
            g = np.array([R.spec().rpspec_g(r["lS"][0, i], r["M"][0, i], CP[p], CF[p]) for i in range(7)])
            j = int(r["j"][0, p])
            assert j == int(np.argmin(g))
            interior = (p == 0 and name in R.INTERIOR_10) or (p == 1 and name in ("erlang6", "gapped6"))
            if interior:
                k = int(np.argmax(D >= 0))
                assert 0 < k and np.all(D[:k] < 0) and np.all(D[k:] >= 0), (name, p, D)
                assert r["flags"][0, p] == 0 and j in (k - 1, k)
                assert ages[k - 1] <= r["lo"][0, p] < r["hi"][0, p] <= ages[k]
                assert r["nev"][0, p] == 64 * 7 + 1
                assert r["g"][0, p] <= g[j] and r["g"][0, p] < CF[p] / m
                if p == 1:
                    assert abs(r["t"][0, p] / m - 1.40) < 0.01, (name, r["t"][0, p] / m)
            else:
                assert np.all(D < 0), (name, p, D)
                assert r["flags"][0, p] == (R.F_EDGE | R.F_NEVER) and j == 6
                assert np.isinf(r["t"][0, p]) and r["g"][0, p] == CF[p] / m and g[6] >= CF[p] / m
                assert r["lo"][0, p] == r["hi"][0, p] == ages[6] and r["nev"][0, p] == 0


def test_flag_paths():
    S, s = R.named("erlang6")
    m = R.mean(S, s)
    # EDGE without NEVER: the first three ages only
    r = R.replace([S], [s], m * R.GRID[:3], [1.0], [10.0])
    assert r["flags"][0, 0] == R.F_EDGE and r["t"][0, 0] == m * R.GRID[2] and r["j"][0, 0] == 2
    assert r["g"][0, 0] < 10.0 / m and r["lo"][0, 0] == r["hi"][0, 0] == r["t"][0, 0] and r["nev"][0, 0] == 0
    # the first age already past the optimum: the bracket starts at 0
    r = R.replace([S], [s], m * R.GRID[4:], [1.0], [10.0])
    full = R.replace([S], [s], m * R.GRID, [1.0], [10.0])
    assert r["flags"][0, 0] == 0 and r["j"][0, 0] == 0 and r["hi"][0, 0] <= m * R.GRID[4]
    assert abs(r["t"][0, 0] / full["t"][0, 0] - 1) < 2.0 ** -38 and r["lo"][0, 0] > 0
    # unusable pairs beside a usable one
    cp, cf = [1.0, 2.0, 0.0, 1.0, np.nan, -1.0, 1.0], [10.0, 1.0, 1.0, np.inf, 2.0, 2.0, 1.0]
    r = R.replace([S], [s], m * R.GRID, cp, cf)
    assert r["flags"][0, 0] == 0 and np.all(r["flags"][0, 1:] == R.F_COST)
    assert np.all(np.isnan(r["t"][0, 1:])) and np.all(np.isnan(r["g"][0, 1:])) and np.all(r["j"][0, 1:] == -1)
    # a flagged and a trapped draw
    Sn, St, st = S.copy(), S.copy(), s.copy()
    Sn[2, 2] = np.nan
    St[0, 1:] = 0.0
    r = R.replace([Sn, St], [s, st], m * R.GRID, [1.0], [10.0])
    assert r["draw_flags"][0] != 0 and r["draw_flags"][1] == R.F_TRAP and np.all(np.isnan(r["m"]))
    assert np.all(r["flags"] == R.F_DRAW) and np.all(r["age_flags"] == R.A_DRAW)
    assert np.all(np.isnan(r["t"])) and np.all(np.isnan(r["M"])) and np.all(r["j"] == -1)
    # no good age: every age beyond mu tau = 1400
    mu = float(np.max(-np.diag(S)))
    r = R.replace([S], [s], np.array([2000.0, 3000.0]) / mu, [1.0], [10.0])
    assert np.all(r["age_flags"] == R.A_BEYOND) and r["flags"][0, 0] == R.F_NOAGE and np.isnan(r["t"][0, 0])
    assert r["draw_flags"][0] == 0 and r["m"][0] == m
    # UNREFINED, the lower end: D >= 0 at the argmin and at its lower neighbour (two local minima)
    S2, s2 = R.bimodal(0.3)
    m2 = R.mean(S2, s2)
    a = m2 * np.array([0.125, 1.2])
    r = R.replace([S2], [s2], a, [1.0], [10.0])
    D = [R.spec().rpspec_D(r["lS"][0, i], r["lf"][0, i], r["M"][0, i], 1.0, 10.0) for i in range(2)]
    assert D[0] >= 0 and D[1] >= 0 and r["j"][0, 0] == 1
    assert r["flags"][0, 0] == R.F_UNREFINED and r["t"][0, 0] == a[1] and r["lo"][0, 0] == r["hi"][0, 0] == a[1]
    assert r["g"][0, 0] == R.spec().rpspec_g(r["lS"][0, 1], r["M"][0, 1], 1.0, 10.0) and r["nev"][0, 0] == 0
    # UNREFINED, the upper end: D < 0 at the argmin and at its upper neighbour
    S3, s3 = R.bimodal(0.5)
    m3 = R.mean(S3, s3)
    a = m3 * np.array([0.05, 1.0, 3.0])
    r = R.replace([S3], [s3], a, [1.0], [30.0])
    D = [R.spec().rpspec_D(r["lS"][0, i], r["lf"][0, i], r["M"][0, i], 1.0, 30.0) for i in range(3)]
    assert D[0] < 0 and D[1] < 0 and r["j"][0, 0] == 0
    assert r["flags"][0, 0] == R.F_UNREFINED and r["t"][0, 0] == a[0] and r["nev"][0, 0] == 0
    # the same draw on a grid that resolves both minima: the global one, refined
    fine = m3 * np.geomspace(0.02, 5.0, 40)
    r = R.replace([S3], [s3], fine, [1.0], [30.0])
    assert r["flags"][0, 0] == 0 and abs(r["t"][0, 0] / m3 - 0.059) < 0.003


def test_a_bad_evaluation_inside_the_bracket_is_EVAL():
    """pht_rp_policy at unit level on a table cut to three rows: the curve's
    ages stay good, every point inside the bracket is bad (the upward sweep
    reaches the table's end), so the first multisection step ends the search:
    NaN, PHT_RP_F_EVAL, the grid cell in lo / hi, 64 points.  With every row
    the same call is pht_rp_draw's policy bit for bit.  (PHT_RP_F_CAP needs 400
    steps; two doubles are never that many multisections apart, so nothing
    reaches it.)"""
    S, s = R.named("erlang6")
    ages = R.mean(S, s) * R.GRID
    full = R.replace([S], [s], ages, [1.0], [10.0])
    same = R.policy_K(S, s, ages, 1.0, 10.0, 4096)
    for k in ("t", "g", "lo", "hi"):
        assert same[k] == full[k][0, 0], k
    assert (same["j"], same["nev"], same["flags"]) == (full["j"][0, 0], full["nev"][0, 0], 0)
    cut = R.policy_K(S, s, ages, 1.0, 10.0, 3)
    assert cut["flags"] == R.F_EVAL and np.isnan(cut["t"]) and np.isnan(cut["g"])
    assert cut["j"] == full["j"][0, 0] == 3 and cut["nev"] == 64
    assert (cut["lo"], cut["hi"]) == (ages[2], ages[3])


def test_points_per_root_on_a_fine_grid():
    """a cell of a 300-age grid is 1.8 % wide: six multisection steps, 385
    points; a cell of the seven-age grid takes seven, 449 (the largest nev)"""
    for name in ("bd10", "hypoexp6"):
        S, s = R.named(name)
        m = R.mean(S, s)
        r = R.replace([S], [s], m * np.geomspace(0.02, 4.0, 300), [1.0], [10.0])
        assert r["flags"][0, 0] == 0 and r["nev"][0, 0] == 64 * 6 + 1, (name, r["nev"])
        r7 = R.replace([S], [s], m * R.GRID, [1.0], [10.0])
        assert r7["nev"][0, 0] == 64 * 7 + 1 and abs(r["t"][0, 0] / r7["t"][0, 0] - 1) < 2.0 ** -38


def _chain_result():
    """bd3 at five scalings, a NaN draw, reversible6-like NEVER comes from the
    pair (1, 1.5); erlang-like EDGE from a short grid is a case of its own"""
    S, s = R.named("bd3")
    scales = (0.8, 0.9, 1.0, 1.1, 1.25)
    Ss, ss = [S * c for c in scales], [s * c for c in scales]
    Sn = S.copy()
    Sn[0, 0] = np.nan
    Ss.append(Sn)
    ss.append(s)
    ages = R.mean(S, s) * R.GRID
    return Ss, ss, ages, R.replace(Ss, ss, ages, CP, CF)


def test_summary_counts_add_up_and_bayes_age():
    import phasetype_amd as P

    Ss, ss, ages, r = _chain_result()
    out = P.replacement_summary(r, ages, CP, CF)
    tot = out["n_finite"] + out["n_never"] + out["n_edge"] + out["n_flagged"]
    assert np.array_equal(tot, [6, 6])
    assert np.array_equal(out["n_flagged"], [1, 1]) and np.array_equal(out["n_finite"], [5, 0])
    assert np.array_equal(out["n_never"], [0, 5]) and np.array_equal(out["n_edge"], [0, 0])
    assert np.all(np.diff(out["band"][:, 0]) >= 0) and np.all(np.isnan(out["band"][:, 1]))
    assert np.all(out["saving"][:5, 0] > 0) and np.all(out["saving"][:5, 1] == 0) and np.all(np.isnan(out["saving"][5]))
    assert out["gbar"].shape == (2, 7) and out["n_bad_ages"] == 0 and np.all(np.isfinite(out["gbar"]))
    assert out["evpi"][0] >= 0 and out["age_bayes"][0] in ages
    # a short grid: EDGE without NEVER is counted as such
    S, s = R.named("erlang6")
    a3 = R.mean(S, s) * R.GRID[:3]
    o3 = P.replacement_summary(R.replace([S, S], [s, s], a3, [1.0], [10.0]), a3, [1.0], [10.0])
    assert o3["n_edge"][0] == 2 and o3["n_finite"][0] == 0 and o3["n_never"][0] == 0 and o3["n_flagged"][0] == 0
    # an age that is bad for one unflagged draw is NaN in gbar and counted
    mu = float(np.max(-np.diag(S)))
    a2 = np.array([1.0, 1000.0 / mu])
    o2 = P.replacement_summary(R.replace([S, 2 * S], [s, 2 * s], a2, [1.0], [10.0]), a2, [1.0], [10.0])
    assert o2["n_bad_ages"] == 1 and np.isnan(o2["gbar"][0, 1]) and np.isfinite(o2["gbar"][0, 0])
    # identical draws: the Bayes age is the grid's argmin, and knowing the parameters saves what refining does
    S, s = R.named("bd10")
    ages = R.mean(S, s) * R.GRID
    r = R.replace([S] * 4, [s] * 4, ages, CP, CF)
    o = P.replacement_summary(r, ages, CP, CF)
    assert np.array_equal(o["age_bayes"], ages[r["j"][0]])
    g0 = R.spec().rpspec_g(r["lS"][0, r["j"][0, 0]], r["M"][0, r["j"][0, 0]], 1.0, 10.0)
    assert abs(o["g_bayes"][0] - g0) <= 4 * np.spacing(g0) and abs(o["evpi"][0] - (g0 - r["g"][0, 0])) <= 1e-14


def test_fleet_overdue_against_a_brute_force_loop():
    import phasetype_amd as P

    rng = np.random.default_rng(9)
    t = rng.uniform(0.5, 3.0, (5, 2))
    t[1, 0], t[2, 0], t[3, 1] = np.inf, np.nan, 1.5
    c = np.array([0.2, 1.5, 1.5, 2.9, 0.7, 3.5, 1.0, 2.2, 0.5])
    c[3] = t[0, 0]  # a unit exactly at a draw's optimal age is overdue
    bayes = np.array([1.5, np.nan])
    out = P.replacement_overdue(t, bayes, c)
    for p in range(2):
        ok = [d for d in range(5) if not np.isnan(t[d, p])]
        for u in range(9):
            share = sum(1 for d in ok if t[d, p] <= c[u]) / len(ok)
            assert out["p_overdue"][p, u] == share, (p, u)
        for d in range(5):
            if d in ok:
                assert out["n_overdue"][d, p] == sum(1 for u in range(9) if c[u] >= t[d, p])
            else:
                assert np.isnan(out["n_overdue"][d, p])
    assert out["n_overdue"][1, 0] == 0  # never replace: no unit is overdue
    assert out["n_overdue_bayes"][0] == sum(1 for u in range(9) if c[u] >= 1.5) and out["n_overdue_bayes"][1] == 0
    assert out["n_overdue_band"].shape == (3, 2)


def test_library_host_function_is_the_restatement(lib):
    import phasetype_amd as P

    for name, G, cp, cf in (("bd3", R.GRID, CP, CF), ("erlang6", R.GRID[:3], [1.0], [10.0]),
                            ("neareq12", np.geomspace(0.02, 4.0, 300), CP, CF), ("stiff6", R.GRID, CP, CF)):
        S, s = R.named(name)
        ages = R.mean(S, s) * np.asarray(G)
        want = R.replace([S], [s], ages, cp, cf)
        got = P.replace_host(S, s, ages, cp, cf)
        for k in R.FLOATS + R.POINT_F:
            assert np.array_equal(np.asarray(got[k], np.float64).reshape(-1).view(np.uint64),
                                  want[k][0].reshape(-1).view(np.uint64)), (name, k)
        for k in ("j", "nev", "flags", "age_flags"):
            assert np.array_equal(got[k], want[k][0]), (name, k)
        assert got["draw_flags"] == want["draw_flags"][0]
    S, s = R.named("bd3")
    Sn = S.copy()
    Sn[1, 1] = np.nan
    got = P.replace_host(Sn, s, [1.0], [1.0], [2.0])
    assert got["bad_draw"] and got["flags"][0] == P.RP_F_DRAW and np.isnan(got["m"])
    assert (P.RP_F_COST, P.RP_F_DRAW, P.RP_F_NOAGE, P.RP_F_UNREFINED, P.RP_F_EDGE, P.RP_F_EVAL, P.RP_F_NEVER,
            P.RP_F_CAP) == (R.F_COST, R.F_DRAW, R.F_NOAGE, R.F_UNREFINED, R.F_EDGE, R.F_EVAL, R.F_NEVER, R.F_CAP)
    # refusals, each with its message
    for ages, cp, cf, msg in (([1.0, 1.0], [1.0], [2.0], "strictly increasing"), ([0.0, 1.0], [1.0], [2.0], "positive"),
                              ([1.0, np.inf], [1.0], [2.0], "finite"), (np.arange(1.0, 1026.0), [1.0], [2.0], "1024"),
                              ([], [1.0], [2.0], "ages"), ([1.0], np.ones(17), 2 * np.ones(17), "cost pairs"),
                              ([1.0], [], [], "cost pairs")):
        with pytest.raises(P.PhaseTypeError, match=msg):
            P.replace_host(S, s, ages, cp, cf)
    with pytest.raises(P.PhaseTypeError, match="n <= 32"):
        P.replace_host(-np.eye(33), np.ones(33), [1.0], [1.0], [2.0])
