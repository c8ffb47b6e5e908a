"""The tests' CPU restatement of include/pht_condition.h (tests/condition_spec.c,
compiled here with ``cc -O2 -ffp-contract=off`` into a shared object in a
temporary directory) behind numpy wrappers that give ``Sweeper.condition``'s
dict, the header's contract for phi, and the truth (mpmath: the first row of
exp(S c) through tests/evaluator_cases, m by a linear solve, r_h by the
augmented-matrix integral).  Shared by tests/test_condition.py and
tests/test_gpu_condition.py."""
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
_ip = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_SPEC = None

KEYS = ("words", "scales", "phisum", "mrlsum", "dsum", "cnt", "unit_index", "flags", "bad_draw")
POINT = ("phi", "mrl", "d")
DERIVED = ("Phi", "L", "Delta", "nbad", "nunits", "p_phase", "mrl_unit", "demand_unit")


def spec():
    global _SPEC
    if _SPEC is None:
        td = tempfile.mkdtemp(prefix="pht_condition_spec_")
        atexit.register(shutil.rmtree, td, ignore_errors=True)
        so = os.path.join(td, "condition_spec.so")
        cc = shutil.which("cc") or shutil.which("gcc")
        subprocess.run([cc, "-O2", "-ffp-contract=off", "-shared", "-fPIC", f"-I{os.path.join(REPO, 'include')}",
                        "-o", so, os.path.join(HERE, "condition_spec.c"), "-lm"], check=True)
        L = C.CDLL(so)
        L.cspec_maxunits.restype = C.c_long
        L.cspec_scale.restype = L.cspec_m_r.restype = L.cspec_r_r.restype = C.c_double
        L.cspec_f_trap.restype = L.cspec_f_hcap.restype = C.c_uint
        L.cspec_horizons_ok.argtypes = [C.c_int, _dp]
        L.cspec_phi_bound.argtypes = [C.c_int, C.c_int, C.c_double]
        L.cspec_phi_bound.restype = C.c_double
        L.cspec_r_bound.argtypes = [C.c_double]
        L.cspec_r_bound.restype = C.c_double
        L.cspec_mean.argtypes = [C.c_int, _dp, _dp, _dp]
        L.cspec_mean.restype = C.c_uint
        L.cspec_renewal.argtypes = [C.c_int, _dp, _dp, C.c_double, C.c_int, _dp, _dp, C.POINTER(C.c_int)]
        L.cspec_renewal.restype = C.c_uint
        L.cspec_windows.argtypes = [C.c_int, _dp, _dp, C.c_long, _dp, C.c_double, _dp, _ip, _ip]
        L.cspec_windows.restype = None
        L.cspec_draw.argtypes = [C.c_int, _dp, _dp, C.c_long, _dp, C.c_double, C.c_int, _dp, _lp, _dp] + \
            [C.c_void_p] * 7
        L.cspec_draw.restype = C.c_uint
        _SPEC = L
    return _SPEC


def _flat(S, s):
    S = np.asarray(S, np.float64)
    return S.shape[0], np.ascontiguousarray(S.reshape(-1, order="F")), np.ascontiguousarray(s, np.float64)


def units(y, censored):
    """(unit_index, ages): the censored observations in the caller's order"""
    idx = np.flatnonzero(np.asarray(censored) != 0).astype(np.int64)
    return idx, np.ascontiguousarray(np.asarray(y, np.float64)[idx])


def mean(S, s):
    """(m, flag) of pht_cd_mean"""
    n, Sf, sf = _flat(S, s)
    m = np.zeros(n)
    return m, int(spec().cspec_mean(n, Sf, sf, m))


def renewal(S, s, horizons):
    """(r [H, n], Kr, flag) of pht_cd_renewal"""
    n, Sf, sf = _flat(S, s)
    h = np.ascontiguousarray(np.atleast_1d(horizons), np.float64)
    r = np.zeros((len(h), n))
    Kr = C.c_int(0)
    f = int(spec().cspec_renewal(n, Sf, sf, float(np.max(-np.diag(np.asarray(S)))), len(h), h, r, C.byref(Kr)))
    return r, Kr.value, f


def windows(S, s, ages, ymax_c=None):
    """(l, bad, khi) per unit: pht_es_window's, the table sized for ymax_c"""
    n, Sf, sf = _flat(S, s)
    ages = np.ascontiguousarray(ages, np.float64)
    l, bad, khi = np.full(len(ages), np.nan), np.zeros(len(ages), np.int32), np.zeros(len(ages), np.int32)
    spec().cspec_windows(n, Sf, sf, len(ages), ages, float(np.max(ages) if ymax_c is None else ymax_c), l, bad, khi)
    return l, bad, khi


def finalise(words, scales, phisum, mrlsum, dsum, cnt, idx, flags, phi=None, mrl=None, d=None):
    """Sweeper.condition's dict from the raw outputs, restated"""
    words = np.asarray(words, np.int64)
    n, nh = phisum.shape[1], dsum.shape[1]
    k = np.maximum(cnt, 1).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        p_phase = np.where(cnt[:, None] > 0, phisum / k[:, None], np.nan)
        mrl_unit = np.where(cnt > 0, mrlsum / k, np.nan)
        demand_unit = np.where(cnt[:, None] > 0, dsum / k[:, None], np.nan)
    out = dict(Phi=words[:, :n] * 2.0 ** -40, L=(words[:, n] * 2.0 ** -40) * scales[:, 0],
               Delta=(words[:, n + 1:n + 1 + nh] * 2.0 ** -40) * scales[:, 1:], nbad=words[:, n + nh + 1].copy(),
               nunits=words[:, n + nh + 2].copy(), words=words, scales=scales, phisum=phisum, mrlsum=mrlsum,
               dsum=dsum, cnt=cnt, p_phase=p_phase, mrl_unit=mrl_unit, demand_unit=demand_unit, unit_index=idx,
               bad_draw=np.asarray(flags) != 0, flags=np.asarray(flags, np.int32))
    if phi is not None:
        out.update(phi=phi, mrl=mrl, d=d)
    return out


def condition(S_list, s_list, y, censored, horizons=None, ymax_c=None, pointwise=True):
    """Sweeper.condition's dict from the restatement, for a context holding
    (y, censored); ymax_c: the largest censored observation the tables are
    sized for (default: this context's)"""
    idx, ages = units(y, censored)
    h = np.ascontiguousarray(np.atleast_1d([] if horizons is None else horizons), np.float64).reshape(-1)
    nd, nc, nh = len(S_list), len(ages), len(h)
    n = np.asarray(S_list[0]).shape[0]
    assert spec().cspec_horizons_ok(nh, h if nh else np.zeros(1)) and nc >= 1
    ymax_c = float(np.max(ages)) if ymax_c is None else float(ymax_c)
    words, scales = np.zeros((nd, n + nh + 3), np.int64), np.zeros((nd, 1 + nh))
    phisum, mrlsum, dsum, cnt = np.zeros((nc, n)), np.zeros(nc), np.zeros((nc, nh)), np.zeros(nc, np.int64)
    phi = np.zeros((nd, nc, n)) if pointwise else None
    mrl = np.zeros((nd, nc)) if pointwise else None
    d = np.zeros((nd, nc, nh)) if pointwise else None
    flags = np.zeros(nd, np.int32)
    for k, (S, s) in enumerate(zip(S_list, s_list)):
        _, Sf, sf = _flat(S, s)
        flags[k] = spec().cspec_draw(n, Sf, sf, nc, ages, ymax_c, nh, h if nh else np.zeros(1), words[k], scales[k],
                                     phisum.ctypes.data, mrlsum.ctypes.data, dsum.ctypes.data, cnt.ctypes.data,
                                     phi[k].ctypes.data if pointwise else None,
                                     mrl[k].ctypes.data if pointwise else None,
                                     d[k].ctypes.data if pointwise else None)
    return finalise(words, scales, phisum, mrlsum, dsum, cnt, idx, flags, phi, mrl, d)


def same_bits(a, b, keys=KEYS + POINT + DERIVED):
    """the keys of two condition dicts whose bytes differ (NaN payloads included)"""
    bad = []
    for k in keys:
        if k not in a and k not in b:
            continue
        x, w = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != w.shape or x.dtype != w.dtype or x.tobytes() != w.tobytes():
            bad.append(k)
    return bad


# --------------------------------------------------------------------- truth
def truth_phi(S, ages):
    """phi[unit][j] as mpmath numbers: the first row of exp(S c) over its sum
    (evaluator_cases._row: the working precision grows with n, 1 / c and mu c)"""
    import mpmath as mp

    import evaluator_cases as E

    S = np.ascontiguousarray(S, np.float64)
    out = []
    for c in ages:
        if float(c) == 0.0:
            out.append([mp.mpf(1 if j == 0 else 0) for j in range(S.shape[0])])
            continue
        row, dps = E._row(S, float(c))
        with mp.workdps(dps):
            tot = mp.fsum(row)
            out.append([v / tot for v in row])
    return out


def truth_m(S, dps=60):
    """m = (-S)^-1 1 as mpmath numbers.  Every m_i is a mean time to absorption,
    at least 1 / mu, and the solve's error is relative to the largest of them
    times the condition number: 60 digits, with the residual checked to 30
    digits below the smallest m_i"""
    import mpmath as mp

    with mp.workdps(dps):
        A = -mp.matrix(np.asarray(S, np.float64).tolist())
        one = mp.ones(A.rows, 1)
        m = mp.lu_solve(A, one)
        res = mp.norm(A * m - one, mp.inf)
        amax = max(mp.fabs(A[i, j]) for i in range(A.rows) for j in range(A.cols))
        assert min(m) > 0 and res <= mp.mpf(10) ** (30 - dps) * amax * min(m), \
            ("the working precision does not resolve m", dps, float(res))
        return list(m)


def truth_r_dps(n, x):
    """the working precision of truth_r at x = mu h: r_h[i] is as small as
    (mu h)^(n - i) on a chain and expm's error is absolute, so
    60 + ceil(3 n max(0, -log10 x)) + x / 2.3 digits (evaluator_cases._dps's
    growth)"""
    import math

    small = math.ceil(3 * n * max(0.0, -math.log10(x))) if x > 0 else 0
    return int(60 + small + int(x / 2.3))


def truth_r(S, s, horizons, dps=None):
    """r_h[i] = (int_0^h exp(Q* u) s du)_i, Q* = S + s e_1^T, as mpmath numbers:
    the last column of exp([[Q*, s], [0, 0]] h), at truth_r_dps digits (dps: a
    fixed precision instead, for the test of the guard); a value that the
    working precision does not resolve by 30 digits fails here"""
    import mpmath as mp

    S = np.asarray(S, np.float64)
    n = S.shape[0]
    mu = float(np.max(-np.diag(S)))
    out = []
    for h in horizons:
        wp = truth_r_dps(n, mu * float(h)) if dps is None else int(dps)
        with mp.workdps(wp):
            M = mp.zeros(n + 1, n + 1)
            for i in range(n):
                for j in range(n):
                    M[i, j] = mp.mpf(float(S[i, j]))
                M[i, 0] += mp.mpf(float(s[i]))
                M[i, n] = mp.mpf(float(s[i]))
            E = mp.expm(M * mp.mpf(float(h)))
            out.append([E[i, n] for i in range(n)])
            if float(h) > 0:
                assert all(v > mp.mpf(10) ** (30 - wp) for v in out[-1]), \
                    ("the working precision does not resolve this r_h", float(h), wp, float(min(out[-1])))
    return out


def phi_bound(n, khi, phi_true):
    """the header's contract per [unit, j]"""
    khi = np.asarray(khi)
    return np.array([[spec().cspec_phi_bound(int(n), int(k), float(p)) for p in row]
                     for k, row in zip(khi, phi_true)])
