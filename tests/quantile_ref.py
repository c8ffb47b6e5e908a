"""The tests' CPU restatement of include/pht_quantile.h (tests/quantile_spec.c,
compiled here with ``cc -O2 -ffp-contract=off`` into a shared object in a
temporary directory; the evaluator is tests/loglik_unif_ref.py's) behind numpy
wrappers, the header's error bound, and the high-precision reference (mpmath,
50 digits).  Shared by tests/test_quantile.py and tests/test_gpu_quantile.py."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import loglik_unif_ref as U

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

_dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_ip = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_up = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
_SPEC = None

F_P, F_T0, F_BEYOND, F_EVAL, F_CAP, F_DRAW = 1, 2, 4, 8, 16, 32
KEYS = ("t", "lo", "hi", "nev", "flags", "bad_draw")


def spec():
    global _SPEC
    if _SPEC is None:
        td = tempfile.mkdtemp(prefix="pht_quantile_spec_")
        atexit.register(shutil.rmtree, td, ignore_errors=True)
        so = os.path.join(td, "quantile_spec.so")
        cc = shutil.which("cc") or shutil.which("gcc")
        subprocess.run([cc, "-O2", "-ffp-contract=off", "-shared", "-fPIC", f"-I{os.path.join(REPO, 'include')}",
                        "-o", so, os.path.join(HERE, "quantile_spec.c"), "-lm"], check=True)
        L = C.CDLL(so)
        L.qspec_lambda.restype = L.qspec_rtol.restype = C.c_double
        L.qspec_stop.argtypes = [C.c_double, C.c_double]
        L.qspec_L.argtypes = [C.c_double, C.c_double]
        L.qspec_L.restype = C.c_double
        L.qspec_meta.argtypes = [C.c_int, _dp, _dp, C.c_double, _dp, _dp]
        L.qspec_meta.restype = C.c_uint
        L.qspec_draw.argtypes = [C.c_int, _dp, _dp, C.c_int, _dp, C.c_double, C.c_double, _dp, _dp, _dp, _ip, _up]
        L.qspec_draw.restype = C.c_uint
        _SPEC = L
    return _SPEC


def _flat(S, s):
    S = np.asarray(S, np.float64)
    return S.shape[0], np.ascontiguousarray(S.reshape(-1, order="F")), np.ascontiguousarray(s, np.float64)


def meta(S, s, tmax=np.inf):
    """dict(flag, mu, abar, K, thi) of one draw"""
    n, Sf, sf = _flat(S, s)
    m, thi = np.zeros(4), np.zeros(1)
    flag = int(spec().qspec_meta(n, Sf, sf, float(tmax), m, thi))
    return dict(flag=flag, mu=m[1], abar=m[2], K=int(m[3]), thi=float(thi[0]))


def quantile(S_list, s_list, probs, given=0.0, tmax=np.inf):
    """Sweeper.quantile's dict from the restatement: t, lo, hi (float64),
    nev (int32), flags (uint32), each [draws, P], and bad_draw [draws]"""
    probs = np.ascontiguousarray(np.atleast_1d(probs), np.float64)
    nd, P = len(S_list), len(probs)
    out = dict(t=np.zeros((nd, P)), lo=np.zeros((nd, P)), hi=np.zeros((nd, P)), nev=np.zeros((nd, P), np.int32),
               flags=np.zeros((nd, P), np.uint32), bad_draw=np.zeros(nd, bool), draw_flags=np.zeros(nd, np.int32))
    for d, (S, s) in enumerate(zip(S_list, s_list)):
        n, Sf, sf = _flat(S, s)
        f = spec().qspec_draw(n, Sf, sf, P, probs, float(given), float(tmax), out["t"][d], out["lo"][d], out["hi"][d],
                              out["nev"][d], out["flags"][d])
        out["draw_flags"][d] = f
        out["bad_draw"][d] = f != 0
    return out


def logsurv(S, s, t, tmax=np.inf):
    """(lS, khi) at the times t from the draw's quantile table (the table the
    root search used: K from the draw's horizon)"""
    m = meta(S, s, tmax)
    t = np.ascontiguousarray(np.atleast_1d(t), np.float64)
    l, khi = U.pointwise([S], [s], t, np.ones(len(t), np.int32), ymax=m["thi"], with_khi=True)
    return l[0], khi[0]


def target(S, s, p, given=0.0, tmax=np.inf):
    """L per probability, the header's bits (lS(t0) from the draw's table)"""
    l0 = float(logsurv(S, s, [given], tmax)[0][0]) if given > 0 else 0.0
    return np.array([spec().qspec_L(float(v), l0) for v in np.atleast_1d(p)])


def stop_holds(lo, hi):
    return np.array([bool(spec().qspec_stop(float(a), float(b))) for a, b in zip(np.atleast_1d(lo), np.atleast_1d(hi))])


def hazard(S, s, t, tmax=np.inf):
    """exp(lf - lS) at the times t from the draw's quantile table"""
    m = meta(S, s, tmax)
    t = np.ascontiguousarray(np.atleast_1d(t), np.float64)
    lf = U.pointwise([S], [s], t, np.zeros(len(t), np.int32), ymax=m["thi"])[0]
    return np.exp(lf - logsurv(S, s, t, tmax)[0])


def log1p_neg(p):
    return np.log1p(-np.asarray(p, np.float64))


def bound(S, s, p, lo, hi, given=0.0, tmax=np.inf):
    """the header's bound on |log Fbar_true(t^) - L| for finite roots"""
    n = np.asarray(S).shape[0]
    m = meta(S, s, tmax)
    la, ka = logsurv(S, s, lo, tmax)
    lb, kb = logsurv(S, s, hi, tmax)
    e0, l0 = 0.0, 0.0
    if given > 0:
        l0v, k0 = logsurv(S, s, [given], tmax)
        e0, l0 = float(U.bound(n, k0)[0]), float(l0v[0])
    lp = log1p_neg(p)
    dL = 2.0 ** -50 * np.abs(lp) + 2.0 ** -53 * np.abs(lp + l0)
    return U.bound(n, ka) + U.bound(n, kb) + e0 + m["abar"] * (np.asarray(hi) - np.asarray(lo)) + dL


def mp_logsurv(S, t, dps=50):
    """log(e_1^T expm(S t) 1) as mpmath numbers"""
    import mpmath as mp

    S = np.asarray(S, np.float64)
    n = S.shape[0]
    with mp.workdps(dps):
        M = mp.matrix(n, n)
        for i in range(n):
            for j in range(n):
                M[i, j] = mp.mpf(float(S[i, j]))
        out = []
        for tv in np.atleast_1d(t):
            X = mp.expm(M * mp.mpf(float(tv)))
            out.append(mp.log(sum(X[0, j] for j in range(n))))
        return out
