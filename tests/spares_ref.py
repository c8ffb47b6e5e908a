"""The tests' CPU restatement of include/pht_spares.h (tests/spares_spec.c,
compiled here with ``cc -O2 -ffp-contract=off`` into a shared object in a
temporary directory) behind numpy wrappers that give ``Sweeper.spares``'s
dict, and the truth (mpmath: the first and second factorial moments of the
replacement count from exp of the augmented generator).  Shared by
tests/test_spares.py and tests/test_gpu_spares.py."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

_dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_lp = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
_SPEC = None

KEYS = ("words", "scales", "dsum", "vsum", "d2sum", "cnt", "unit_index", "flags", "bad_draw")
POINT = ("d", "var")
DERIVED = ("Delta", "V", "nbad", "nunits", "demand_unit", "demand_unit_sd")
ALL = KEYS + POINT + DERIVED


def spec():
    global _SPEC
    if _SPEC is None:
        td = tempfile.mkdtemp(prefix="pht_spares_spec_")
        atexit.register(shutil.rmtree, td, ignore_errors=True)
        so = os.path.join(td, "spares_spec.so")
        cc = shutil.which("cc") or shutil.which("gcc")
        subprocess.run([cc, "-O2", "-ffp-contract=off", "-shared", "-fPIC", f"-I{os.path.join(REPO, 'include')}",
                        "-o", so, os.path.join(HERE, "spares_spec.c"), "-lm"], check=True)
        L = C.CDLL(so)
        L.sspec_q_r.restype = L.sspec_v_r.restype = C.c_double
        L.sspec_q_bound.argtypes = [C.c_double]
        L.sspec_q_bound.restype = C.c_double
        L.sspec_var_bound.argtypes = [C.c_double] * 3
        L.sspec_var_bound.restype = C.c_double
        L.sspec_var.argtypes = [C.c_double] * 2
        L.sspec_var.restype = C.c_double
        L.sspec_horizons_ok.argtypes = [C.c_int, _dp]
        L.sspec_vectors.argtypes = [C.c_int, _dp, _dp, C.c_double, C.c_int, _dp, _dp, _dp, _dp, C.POINTER(C.c_int)]
        L.sspec_vectors.restype = C.c_uint
        L.sspec_draw.argtypes = [C.c_int, _dp, _dp, C.c_long, _dp, C.c_double, C.c_int, _dp, _lp, _dp] + \
            [C.c_void_p] * 6
        L.sspec_draw.restype = C.c_uint
        _SPEC = L
    return _SPEC


def _flat(S, s):
    S = np.asarray(S, np.float64)
    return S.shape[0], np.ascontiguousarray(S.reshape(-1, order="F")), np.ascontiguousarray(s, np.float64)


def units(y, censored):
    """(unit_index, ages): the censored observations in the caller's order"""
    idx = np.flatnonzero(np.asarray(censored) != 0).astype(np.int64)
    return idx, np.ascontiguousarray(np.asarray(y, np.float64)[idx])


def vectors(S, s, horizons):
    """(r [H, n], q [H, n], scales [2 H], Kr, flag) of pht_sp_vectors"""
    n, Sf, sf = _flat(S, s)
    h = np.ascontiguousarray(np.atleast_1d(horizons), np.float64)
    r, q, scales = np.zeros((len(h), n)), np.zeros((len(h), n)), np.zeros(2 * len(h))
    Kr = C.c_int(0)
    f = int(spec().sspec_vectors(n, Sf, sf, float(np.max(-np.diag(np.asarray(S)))), len(h), h, r, q, scales,
                                 C.byref(Kr)))
    return r, q, scales, Kr.value, f


def var(D, Q):
    """pht_sp_var, elementwise"""
    D, Q = np.broadcast_arrays(np.asarray(D, np.float64), np.asarray(Q, np.float64))
    out = np.array([spec().sspec_var(float(a), float(b)) for a, b in zip(D.reshape(-1), Q.reshape(-1))])
    return out.reshape(D.shape)


def finalise(words, scales, dsum, vsum, d2sum, cnt, idx, flags, d=None, var=None):
    """Sweeper.spares's dict from the raw outputs, restated"""
    words = np.asarray(words, np.int64)
    nh = dsum.shape[1]
    k = np.maximum(cnt, 1).astype(np.float64)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        demand_unit = np.where(cnt[:, None] > 0, dsum / k, np.nan)
        sd = np.sqrt(np.maximum(vsum / k + d2sum / k - (dsum / k) ** 2, 0.0))
        demand_unit_sd = np.where(cnt[:, None] > 0, sd, np.nan)
    out = dict(Delta=(words[:, :nh] * 2.0 ** -40) * scales[:, :nh],
               V=(words[:, nh:2 * nh] * 2.0 ** -40) * scales[:, nh:], nbad=words[:, 2 * nh].copy(),
               nunits=words[:, 2 * nh + 1].copy(), words=words, scales=scales, dsum=dsum, vsum=vsum, d2sum=d2sum,
               cnt=cnt, demand_unit=demand_unit, demand_unit_sd=demand_unit_sd, unit_index=idx,
               bad_draw=np.asarray(flags) != 0, flags=np.asarray(flags, np.int32))
    if d is not None:
        out.update(d=d, var=var)
    return out


def spares(S_list, s_list, y, censored, horizons, ymax_c=None, pointwise=True):
    """Sweeper.spares's dict from the restatement, for a context holding
    (y, censored); ymax_c: the largest censored observation the tables are
    sized for (default: this context's)"""
    idx, ages = units(y, censored)
    h = np.ascontiguousarray(np.atleast_1d(horizons), np.float64).reshape(-1)
    nd, nc, nh = len(S_list), len(ages), len(h)
    n = np.asarray(S_list[0]).shape[0]
    assert nh >= 1 and spec().sspec_horizons_ok(nh, h) and nc >= 1
    ymax_c = float(np.max(ages)) if ymax_c is None else float(ymax_c)
    words, scales = np.zeros((nd, 2 * nh + 2), np.int64), np.zeros((nd, 2 * nh))
    dsum, vsum, d2sum, cnt = np.zeros((nc, nh)), np.zeros((nc, nh)), np.zeros((nc, nh)), np.zeros(nc, np.int64)
    d = np.zeros((nd, nc, nh)) if pointwise else None
    v = np.zeros((nd, nc, nh)) if pointwise else None
    flags = np.zeros(nd, np.int32)
    for k, (S, s) in enumerate(zip(S_list, s_list)):
        _, Sf, sf = _flat(S, s)
        flags[k] = spec().sspec_draw(n, Sf, sf, nc, ages, ymax_c, nh, h, words[k], scales[k], dsum.ctypes.data,
                                     vsum.ctypes.data, d2sum.ctypes.data, cnt.ctypes.data,
                                     d[k].ctypes.data if pointwise else None, v[k].ctypes.data if pointwise else None)
    return finalise(words, scales, dsum, vsum, d2sum, cnt, idx, flags, d, v)


def same_bits(a, b, keys=ALL):
    """the keys of two spares dicts whose bytes differ (NaN payloads included)"""
    bad = []
    for k in keys:
        if k not in a and k not in b:
            continue
        x, w = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != w.shape or x.dtype != w.dtype or x.tobytes() != w.tobytes():
            bad.append(k)
    return bad


# --------------------------------------------------------------------- truth
def truth_dps(n, x):
    """the working precision of truth_moments at x = mu h:
    60 + ceil(6 n max(0, -log10 x)) + x / 2.3 digits"""
    import math

    small = math.ceil(6 * n * max(0.0, -math.log10(x))) if x > 0 else 0
    return int(60 + small + int(x / 2.3))


def truth_moments(S, s, horizons, dps=None):
    """(M1, M2) per horizon as lists of mpmath numbers per phase: M1 = E_i N(h),
    M2 = E_i N(h) (N(h) - 1), the last column of exp(G h),
    G = [[Q*, 2 s e_1^T, 0], [0, Q*, s], [0, 0, 0]], Q* = S + s e_1^T.  expm's
    error is absolute and on a chain M2[i] is as small as (mu h)^(2 n - i), so
    the digits grow with n and -log10(mu h) as evaluator_cases._dps grows them
    (over the 2 n transient states of G), and with mu h (dps: a fixed precision
    instead, for the test of the guard); a value that the working precision
    does not resolve by 30 digits fails here"""
    import mpmath as mp

    S = np.asarray(S, np.float64)
    n = S.shape[0]
    mu = float(np.max(-np.diag(S)))
    m1, m2 = [], []
    for h in horizons:
        wp = truth_dps(n, mu * float(h)) if dps is None else int(dps)
        with mp.workdps(wp):
            G = mp.zeros(2 * n + 1, 2 * n + 1)
            for i in range(n):
                for j in range(n):
                    G[i, j] = G[n + i, n + j] = mp.mpf(float(S[i, j]))
                si = mp.mpf(float(s[i]))
                G[i, 0] += si
                G[n + i, n] += si
                G[i, n] = 2 * si
                G[n + i, 2 * n] = si
            E = mp.expm(G * mp.mpf(float(h)))
            m2.append([E[i, 2 * n] for i in range(n)])
            m1.append([E[n + i, 2 * n] for i in range(n)])
            if float(h) > 0:
                low = mp.mpf(10) ** (30 - wp)
                assert all(v > low for v in m1[-1] + m2[-1]), \
                    ("the working precision does not resolve this moment", float(h), wp, float(min(m1[-1] + m2[-1])))
    return m1, m2
