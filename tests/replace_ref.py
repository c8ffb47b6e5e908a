"""The tests' CPU restatement of include/pht_replace.h (tests/replace_spec.c,
compiled here with ``cc -O2 -ffp-contract=off`` into a shared object in a
temporary directory) behind numpy wrappers, the header's error bounds, and the
high-precision truths (mpmath, 60 digits and more): the restricted mean
M = m - e_1^T exp(S tau) (-S)^-1 1, D, g and the optimal age by ``findroot``.
Shared by tests/test_replace.py and tests/test_gpu_replace.py."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import evaluator_cases as EC

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

_dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_ip = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_up = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
_SPEC = None

A_BEYOND, A_EVAL, A_DRAW = 1, 2, 4
F_COST, F_DRAW, F_NOAGE, F_UNREFINED, F_EDGE, F_EVAL, F_NEVER, F_CAP = 1, 2, 4, 8, 16, 32, 64, 128
F_TRAP = 64  # PHT_CD_F_TRAP of the draw's flag word
FLOATS = ("t", "g", "lo", "hi", "m")
INTS = ("j", "nev", "flags", "bad_draw", "draw_flags")
POINT_F = ("lS", "lf", "M")
GRID = np.array([0.05, 0.1, 0.2, 0.4, 0.8, 1.6, 3.2])  # ages = m GRID
PAIRS = ((1.0, 10.0), (1.0, 1.5))
# the generators of the issue's table (name -> (family, n, keyword arguments))
NAMED = {"bd3": ("bd", 3, {}), "bd10": ("bd", 10, {}), "erlang6": ("erlang", 6, {}), "acyclic6": ("acyclic", 6, {}),
         "reversible6": ("reversible", 6, {}), "neareq12": ("neareq", 12, {}), "stiff6": ("stiff", 6, {}),
         "hypoexp6": ("hypoexp", 6, {}), "coxian_shared6": ("coxian_shared", 6, {}),
         "gapped6": ("gapped", 6, {"eps": 1e-3})}
# an interior root at (1, 10) on the grid m GRID (stiff6 has none: six of its ages lie beyond mu tau = 1400)
INTERIOR_10 = ("bd3", "bd10", "erlang6", "acyclic6", "neareq12", "hypoexp6", "coxian_shared6", "gapped6")


def spec():
    global _SPEC
    if _SPEC is None:
        td = tempfile.mkdtemp(prefix="pht_replace_spec_")
        atexit.register(shutil.rmtree, td, ignore_errors=True)
        so = os.path.join(td, "replace_spec.so")
        cc = shutil.which("cc") or shutil.which("gcc")
        subprocess.run([cc, "-O2", "-ffp-contract=off", "-shared", "-fPIC", f"-I{os.path.join(REPO, 'include')}",
                        "-o", so, os.path.join(HERE, "replace_spec.c"), "-lm"], check=True)
        L = C.CDLL(so)
        for f in ("rpspec_rtol", "rpspec_M_R", "rpspec_D_R", "rpspec_eps", "rpspec_M_bound", "rpspec_D_bound",
                  "rpspec_g", "rpspec_D"):
            getattr(L, f).restype = C.c_double
        L.rpspec_work.restype = C.c_size_t
        L.rpspec_work.argtypes = [C.c_int]
        L.rpspec_ages_ok.argtypes = [C.c_int, _dp]
        L.rpspec_eps.argtypes = [C.c_int, C.c_int]
        L.rpspec_M_bound.argtypes = [C.c_int, C.c_int, C.c_double]
        L.rpspec_D_bound.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double]
        L.rpspec_g.argtypes = [C.c_double] * 4
        L.rpspec_D.argtypes = [C.c_double] * 5
        L.rpspec_meta.argtypes = [C.c_int, _dp, _dp, C.c_double, _dp, _dp, _dp]
        L.rpspec_meta.restype = C.c_uint
        L.rpspec_eval.argtypes = [C.c_int, _dp, _dp, C.c_double, C.c_int, _dp, _dp, _dp, _dp, _ip, _ip]
        L.rpspec_eval.restype = C.c_uint
        L.rpspec_rmean.argtypes = [C.c_int, _dp, _dp, C.c_double, C.c_int, _dp, _dp, _ip, _ip]
        L.rpspec_rmean.restype = C.c_uint
        L.rpspec_policy_K.argtypes = [C.c_int, _dp, _dp, C.c_int, _dp, C.c_double, C.c_double, C.c_int, _dp, _ip]
        L.rpspec_policy_K.restype = C.c_uint
        L.rpspec_draw.argtypes = [C.c_int, _dp, _dp, C.c_int, _dp, C.c_int, _dp, _dp, _up, _dp, _dp, _dp, _dp, _dp,
                                  _dp, _dp, _dp, _ip, _ip, _up]
        L.rpspec_draw.restype = C.c_uint
        _SPEC = L
    return _SPEC


def _flat(S, s):
    S = np.asarray(S, np.float64)
    return S.shape[0], np.ascontiguousarray(S.reshape(-1, order="F")), np.ascontiguousarray(s, np.float64)


def named(name):
    family, n, kw = NAMED[name]
    return EC.generator(family, n, **kw)


def bimodal(p, k=3, r0=10.0, fast=5.0, slow=0.5):
    """state 1 (rate r0) leads with probability p into a fast Erlang(k) and
    else into a slow one: infant mortality and wear-out, a cost rate with two
    local minima (the PHT_RP_F_UNREFINED paths)"""
    n = 1 + 2 * k
    S, s = np.zeros((n, n)), np.zeros(n)
    S[0, 0], S[0, 1], S[0, 1 + k] = -r0, r0 * p, r0 * (1 - p)
    for base, r in ((1, fast), (1 + k, slow)):
        for i in range(k):
            S[base + i, base + i] = -r
            if i + 1 < k:
                S[base + i, base + i + 1] = r
            else:
                s[base + i] = r
    return S, s


def meta(S, s, tmax):
    """dict(flag, mu, abar, K, thi, m) of one draw"""
    n, Sf, sf = _flat(S, s)
    w, thi, m = np.zeros(4), np.zeros(1), np.zeros(1)
    flag = int(spec().rpspec_meta(n, Sf, sf, float(tmax), w, thi, m))
    return dict(flag=flag, mu=w[1], abar=w[2], K=int(w[3]), thi=float(thi[0]), m=float(m[0]))


def mean(S, s):
    """m = E[T], the header's bits (the grid of a case is m GRID)"""
    return meta(S, s, 1.0)["m"]


def evaluate(S, s, t, tmax=None):
    """dict(lS, lf, M, khi, bad) at the times t from the table sized for tmax
    (default: the largest t)"""
    n, Sf, sf = _flat(S, s)
    t = np.ascontiguousarray(np.atleast_1d(t), np.float64)
    k = len(t)
    out = dict(lS=np.zeros(k), lf=np.zeros(k), M=np.zeros(k), khi=np.zeros(k, np.int32), bad=np.zeros(k, np.int32))
    f = spec().rpspec_eval(n, Sf, sf, float(np.max(t) if tmax is None else tmax), k, t, out["lS"], out["lf"],
                           out["M"], out["khi"], out["bad"])
    assert f == 0, f
    return out


def rmean(S, s, t, tmax=None):
    """dict(M, khi, bad): pht_rp_rmean alone at the times t"""
    n, Sf, sf = _flat(S, s)
    t = np.ascontiguousarray(np.atleast_1d(t), np.float64)
    k = len(t)
    out = dict(M=np.zeros(k), khi=np.zeros(k, np.int32), bad=np.zeros(k, np.int32))
    f = spec().rpspec_rmean(n, Sf, sf, float(np.max(t) if tmax is None else tmax), k, t, out["M"], out["khi"],
                            out["bad"])
    assert f == 0, f
    return out


def policy_K(S, s, ages, cp, cf, Kuse):
    """dict(t, g, lo, hi, j, nev, flags) of pht_rp_policy on the draw's curve
    with only the table's first min(K, Kuse) rows (rpspec_policy_K)"""
    n, Sf, sf = _flat(S, s)
    ages = np.ascontiguousarray(np.atleast_1d(ages), np.float64)
    o4, oi = np.zeros(4), np.zeros(3, np.int32)
    f = spec().rpspec_policy_K(n, Sf, sf, len(ages), ages, float(cp), float(cf), int(Kuse), o4, oi)
    assert f == 0, f
    return dict(t=o4[0], g=o4[1], lo=o4[2], hi=o4[3], j=int(oi[0]), nev=int(oi[1]), flags=int(oi[2]))


def replace(S_list, s_list, ages, cp, cf):
    """Sweeper.replace's dict (pointwise included) from the restatement"""
    ages = np.ascontiguousarray(np.atleast_1d(ages), np.float64)
    cp = np.ascontiguousarray(np.atleast_1d(cp), np.float64)
    cf = np.ascontiguousarray(np.atleast_1d(cf), np.float64)
    nd, G, P = len(S_list), len(ages), len(cp)
    assert spec().rpspec_ages_ok(G, ages) and len(cf) == P
    out = dict(t=np.zeros((nd, P)), g=np.zeros((nd, P)), lo=np.zeros((nd, P)), hi=np.zeros((nd, P)),
               j=np.zeros((nd, P), np.int32), nev=np.zeros((nd, P), np.int32), flags=np.zeros((nd, P), np.uint32),
               m=np.zeros(nd), bad_draw=np.zeros(nd, bool), draw_flags=np.zeros(nd, np.int32),
               lS=np.zeros((nd, G)), lf=np.zeros((nd, G)), M=np.zeros((nd, G)), age_flags=np.zeros((nd, G), np.uint32))
    for d, (S, s) in enumerate(zip(S_list, s_list)):
        n, Sf, sf = _flat(S, s)
        f = spec().rpspec_draw(n, Sf, sf, G, ages, P, cp, cf, out["age_flags"][d], out["lS"][d], out["lf"][d],
                               out["M"][d], out["m"][d:d + 1], out["t"][d], out["g"][d], out["lo"][d], out["hi"][d],
                               out["j"][d], out["nev"][d], out["flags"][d])
        out["draw_flags"][d] = f
        out["bad_draw"][d] = f != 0
    return out


def same_bits(got, want, pointwise=True):
    """the keys on which two results differ in a bit"""
    bad = []
    for k in FLOATS + (POINT_F if pointwise else ()):
        if not np.array_equal(np.ascontiguousarray(got[k], np.float64).view(np.uint64),
                              np.ascontiguousarray(want[k], np.float64).view(np.uint64)):
            bad.append(k)
    for k in INTS + (("age_flags",) if pointwise else ()):
        if not np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)):
            bad.append(k)
    return bad


def M_bound(n, khi, M):
    return spec().rpspec_M_bound(int(n), int(khi), float(M))


def D_bound(n, khi, hM, F, c0):
    return spec().rpspec_D_bound(int(n), int(khi), float(hM), float(F), float(c0))


# --------------------------------------------------------------------- truth
_MV = {}


def _mvec(S):
    """(-S)^-1 1 as mpmath numbers (100 digits)"""
    import mpmath as mp

    key = S.tobytes()
    if key not in _MV:
        with mp.workdps(100):
            A = -mp.matrix(S.tolist())
            _MV[key] = list(mp.lu_solve(A, mp.matrix([1] * S.shape[0])))
    return _MV[key]


def truth(S, s, tau, extra=0):
    """dict(F, Fbar, f, h, M, m) of PH(e_1, S) at tau as mpmath numbers
    (working precision: evaluator_cases' rule plus ``extra`` digits)"""
    import mpmath as mp

    S = np.ascontiguousarray(S, np.float64)
    n = S.shape[0]
    mv = _mvec(S)
    if extra:
        dps = EC._dps(S, float(tau)) + extra
        with mp.workdps(dps):
            E = mp.expm(mp.matrix(S.tolist()) * mp.mpf(tau))
            row = [E[0, j] for j in range(n)]
    else:
        row, dps = EC._row(S, float(tau))
    with mp.workdps(dps + 20):
        Fbar = mp.fsum(row)
        f = mp.fsum(r * mp.mpf(float(c)) for r, c in zip(row, s))
        M = mv[0] - mp.fsum(r * v for r, v in zip(row, mv))
        return dict(F=1 - Fbar, Fbar=Fbar, f=f, h=f / Fbar, M=M, m=mv[0])


def D_true(S, s, tau, cp, cf, extra=0):
    import mpmath as mp

    v = truth(S, s, tau, extra)
    return v["h"] * v["M"] - v["F"] - mp.mpf(float(cp)) / (mp.mpf(float(cf)) - mp.mpf(float(cp)))


def g_true(S, s, tau, cp, cf, extra=0):
    import mpmath as mp

    v = truth(S, s, tau, extra)
    return (mp.mpf(float(cp)) + (mp.mpf(float(cf)) - mp.mpf(float(cp))) * v["F"]) / v["M"]


def root_true(S, s, lo, hi, cp, cf):
    """the zero of D_true by mpmath's findroot from the cell [lo, hi] (a secant
    start at its ends; 40 more digits, the cell is 2^-40 wide)"""
    import mpmath as mp

    with mp.workdps(60):
        a, b = mp.mpf(float(lo)), mp.mpf(float(hi))
        if a == b:
            b = a * (1 + mp.mpf(2) ** -45)
        return mp.findroot(lambda x: D_true(S, s, x, cp, cf, extra=40), (a, b), solver="secant", tol=mp.mpf(10) ** -40,
                           verify=False)
