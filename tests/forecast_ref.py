"""The tests' CPU restatement of include/pht_forecast.h (tests/forecast_spec.c,
compiled here with ``cc -O2 -ffp-contract=off`` into a shared object in a
temporary directory; the evaluator is tests/loglik_unif_ref.py's) behind numpy
wrappers that give ``Sweeper.forecast``'s dict, the header's contract, and the
truth (mpmath, through tests/evaluator_cases.truth).  Shared by
tests/test_forecast.py and tests/test_gpu_forecast.py."""
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
_lp = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
_SPEC = None

KEYS = ("words", "qsum", "cnt", "unit_index", "flags", "bad_draw")


def spec():
    global _SPEC
    if _SPEC is None:
        td = tempfile.mkdtemp(prefix="pht_forecast_spec_")
        atexit.register(shutil.rmtree, td, ignore_errors=True)
        so = os.path.join(td, "forecast_spec.so")
        cc = shutil.which("cc") or shutil.which("gcc")
        subprocess.run([cc, "-O2", "-ffp-contract=off", "-shared", "-fPIC", f"-I{os.path.join(REPO, 'include')}",
                        "-o", so, os.path.join(HERE, "forecast_spec.c"), "-lm"], check=True)
        L = C.CDLL(so)
        L.fspec_maxunits.restype = C.c_long
        L.fspec_thresh.restype = L.fspec_r.restype = L.fspec_scale.restype = C.c_double
        L.fspec_horizons_ok.argtypes = [C.c_int, _dp]
        L.fspec_q.argtypes = [C.c_long, _dp, _dp]
        L.fspec_q.restype = None
        L.fspec_draw.argtypes = [C.c_int, _dp, _dp, C.c_long, _dp, C.c_double, C.c_int, _dp, _lp, C.c_void_p,
                                 C.c_void_p, C.c_void_p]
        L.fspec_draw.restype = C.c_uint
        _SPEC = L
    return _SPEC


def fc_q(dl):
    """pht_fc_q over an array"""
    dl = np.ascontiguousarray(np.atleast_1d(dl), np.float64)
    out = np.zeros(len(dl))
    spec().fspec_q(len(dl), dl, out)
    return out


def units(y, censored):
    """(unit_index, ages): the censored observations in the caller's order"""
    idx = np.flatnonzero(np.asarray(censored) != 0).astype(np.int64)
    return idx, np.ascontiguousarray(np.asarray(y, np.float64)[idx])


def finalise(words, qsum, cnt, idx, flags, q=None):
    """Sweeper.forecast's dict from the raw outputs"""
    words = np.asarray(words, np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        p_unit = np.where(cnt > 0, qsum / np.maximum(cnt, 1), np.nan)
    out = dict(M=words[:, :, 0] * 2.0 ** -40, V=words[:, :, 1] * 2.0 ** -40, nbad=words[:, :, 2].copy(),
               nunits=words[:, :, 3].copy(), words=words, p_unit=p_unit, qsum=qsum, cnt=cnt, unit_index=idx,
               bad_draw=np.asarray(flags) != 0, flags=np.asarray(flags, np.int32))
    if q is not None:
        out["q"] = q
    return out


def forecast(S_list, s_list, y, censored, horizons, ymax_c=None, pointwise=True):
    """Sweeper.forecast's dict from the restatement, for a context holding
    (y, censored); ymax_c: the largest censored observation the tables are
    sized for (default: this context's)"""
    idx, ages = units(y, censored)
    h = np.ascontiguousarray(np.atleast_1d(horizons), np.float64)
    nd, nc, nh = len(S_list), len(ages), len(h)
    assert spec().fspec_horizons_ok(nh, h) and nc >= 1
    ymax_c = float(np.max(ages)) if ymax_c is None else float(ymax_c)
    words = np.zeros((nd, nh, 4), np.int64)
    qsum, cnt = np.zeros((nc, nh)), np.zeros((nc, nh), np.int64)
    q = np.zeros((nd, nc, nh)) if pointwise else None
    flags = np.zeros(nd, np.int32)
    for d, (S, s) in enumerate(zip(S_list, s_list)):
        S = np.asarray(S, np.float64)
        flags[d] = spec().fspec_draw(S.shape[0], np.ascontiguousarray(S.reshape(-1, order="F")),
                                     np.ascontiguousarray(s, np.float64), nc, ages, ymax_c, nh, h, words[d],
                                     qsum.ctypes.data, cnt.ctypes.data, q[d].ctypes.data if pointwise else None)
    return finalise(words, qsum, cnt, idx, flags, q)


def same_bits(a, b, keys=KEYS + ("q",)):
    """the keys of two forecast dicts whose bytes differ (NaN payloads included)"""
    bad = []
    for k in keys:
        if k not in a and k not in b:
            continue
        x, w = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != w.shape or x.dtype != w.dtype or x.tobytes() != w.tobytes():
            bad.append(k)
    return bad


def truth(S, s, ages, horizons):
    """q[unit, horizon] = 1 - Fbar(c + h) / Fbar(c) as mpmath numbers (the log
    survival values are evaluator_cases.truth's, good to more than 30 digits;
    the difference is taken at 80 digits, so q keeps more than 20 even at
    h = 1e-9)"""
    import mpmath as mp

    import evaluator_cases as E

    out = []
    for c in ages:
        l0 = E.truth(S, s, float(c), 1)
        row = []
        for h in horizons:
            if h == 0:
                row.append(mp.mpf(0))
                continue
            lj = E.truth(S, s, float(c) + float(h), 1)  # the double c + h, as the header forms it
            with mp.workdps(80):
                row.append(-mp.expm1(lj - l0))
        out.append(row)
    return out


def bound(S, s, ages, horizons, q_true, ymax_c=None, hmax=None):
    """the header's contract per [unit, horizon]:
    (1 - q) expm1(b(c) + b(c + h) + ulp(dl)) + r q, b the evaluator's bound
    with its ulp(l) (loglik_unif_ref.bound), from the draw's forecast table
    (sized for ymax_c, default the largest age, plus hmax, default the last
    horizon)"""
    ages = np.ascontiguousarray(ages, np.float64)
    h = np.ascontiguousarray(horizons, np.float64)
    n = np.asarray(S).shape[0]
    ymax_c = float(np.max(ages)) if ymax_c is None else float(ymax_c)
    ymax = ymax_c + float(h[-1] if hmax is None else hmax)
    one = np.ones(len(ages), np.int32)
    l0, k0 = U.pointwise([S], [s], ages, one, ymax=ymax, with_khi=True)
    b0 = U.bound(n, k0[0], l0[0])
    out = np.zeros((len(ages), len(h)))
    r = spec().fspec_r()
    for j, hj in enumerate(h):
        lj, kj = U.pointwise([S], [s], ages + hj, one, ymax=ymax, with_khi=True)
        e = b0 + U.bound(n, kj[0], lj[0]) + np.spacing(np.abs(lj[0] - l0[0]))
        qt = np.array([float(v) for v in q_true[:, j]]) if isinstance(q_true, np.ndarray) else \
            np.array([float(row[j]) for row in q_true])
        out[:, j] = (1.0 - qt) * np.expm1(e) + r * qt
    return out


def poisson_binomial(q):
    """the exact law of the number of failures among independent units with
    failure probabilities q (dynamic programming): pmf[0 .. len(q)]"""
    pmf = np.zeros(len(q) + 1)
    pmf[0] = 1.0
    for k, p in enumerate(q):
        pmf[1:k + 2] = pmf[1:k + 2] * (1.0 - p) + pmf[0:k + 1] * p
        pmf[0] *= (1.0 - p)
    return pmf
