"""The tests' CPU restatement of include/pht_loglik_unif.h
(tests/loglik_unif_spec.c, compiled here with ``cc -O2 -ffp-contract=off`` into
a shared object in a temporary directory, as tests/loglik_ref.py compiles its
own) behind numpy wrappers, and the tests' generators with a complex spectrum.
Shared by tests/test_loglik_unif.py and tests/test_gpu_loglik_unif.py; totals
and the WAIC recurrence are loglik_ref's."""
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
_ip = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_SPEC = None

CYCLIC = (np.array([[-1.1, 1, 0], [0, -1.1, 1], [1, 0, -1.1]]), 0.1 * np.ones(3))
SCALES = (0.8, 0.9, 1.0, 1.1, 1.25)
Y_EDGE = [1e-9, 1e-3, 100.0]


def ring(n):
    """bd_exit(n) plus a rate 1.5 from state n back to state 1, the diagonal
    adjusted: a cycle, so a complex spectrum."""
    from phasetype_amd.synth import bd_exit

    S, s = bd_exit(n)
    S[n - 1, 0] += 1.5
    S[n - 1, n - 1] -= 1.5
    return S, s


def scaled(S, s, scales=SCALES):
    return [S * c for c in scales], [s * c for c in scales]


def with_edges(y, cens, edge=Y_EDGE):
    """the observations plus the edge y's, each exact and censored"""
    k = len(edge)
    return (np.concatenate([y, edge, edge]),
            np.concatenate([cens, np.zeros(k, np.int32), np.ones(k, np.int32)]).astype(np.int32))


def spec():
    global _SPEC
    if _SPEC is None:
        td = tempfile.mkdtemp(prefix="pht_loglik_unif_spec_")
        atexit.register(shutil.rmtree, td, ignore_errors=True)
        so = os.path.join(td, "loglik_unif_spec.so")
        cc = shutil.which("cc") or shutil.which("gcc")
        subprocess.run([cc, "-O2", "-ffp-contract=off", "-shared", "-fPIC", f"-I{os.path.join(REPO, 'include')}",
                        "-o", so, os.path.join(HERE, "loglik_unif_spec.c"), "-lm"], check=True)
        L = C.CDLL(so)
        L.uspec_K.argtypes = [C.c_double, C.c_double]
        L.uspec_meta.argtypes = [C.c_int, _dp, _dp, C.c_double, _dp]
        L.uspec_meta.restype = C.c_uint
        L.uspec_table.argtypes = [C.c_int, _dp, _dp, C.c_double, C.c_int, _dp]
        L.uspec_pointwise.argtypes = [C.c_int, C.c_double, C.c_double, _dp, C.c_long, _dp, _ip, _dp, _ip]
        L.uspec_table.restype = L.uspec_pointwise.restype = None
        _SPEC = L
    return _SPEC


def K_of(mu, ymax):
    return spec().uspec_K(float(mu), float(ymax))


def table(S, s, ymax):
    """dict(flag, mu, abar, K, tab [K + 1, 2] = (ax_k, ac_k)) of one draw for a
    context whose largest observation is ymax (tab None for a flagged draw)."""
    S = np.asarray(S, np.float64)
    n = S.shape[0]
    Sf = np.ascontiguousarray(S.reshape(-1, order="F"))
    sf = np.ascontiguousarray(s, np.float64)
    meta = np.zeros(4)
    flag = int(spec().uspec_meta(n, Sf, sf, float(ymax), meta))
    out = dict(flag=flag, mu=meta[1], abar=meta[2], K=int(meta[3]), tab=None)
    if flag == 0:
        tab = np.zeros(2 * (out["K"] + 1))
        spec().uspec_table(n, Sf, sf, out["mu"], out["K"], tab)
        out["tab"] = tab.reshape(-1, 2)
    return out


def pointwise(S_list, s_list, y, cens, ymax=None, with_khi=False):
    """l[draw, observation] (NaN: bad, and every observation of a flagged
    draw); K from ymax (default: the largest of y, as a context holding y)."""
    y = np.ascontiguousarray(y, np.float64)
    cens = np.ascontiguousarray(cens, np.int32)
    ymax = float(np.max(y)) if ymax is None else float(ymax)
    out = np.full((len(S_list), len(y)), np.nan)
    khi = np.zeros((len(S_list), len(y)), np.int32)
    for d, (S, s) in enumerate(zip(S_list, s_list)):
        t = table(S, s, ymax)
        if t["flag"] == 0:
            spec().uspec_pointwise(t["K"], t["mu"], t["abar"], np.ascontiguousarray(t["tab"].reshape(-1)), len(y), y,
                                   cens, out[d], khi[d])
    return (out, khi) if with_khi else out


def bound(n, khi, l=None):
    """the a-priori bound of include/pht_loglik_unif.h on |l - truth|; with
    ``l``, plus one ulp(l): the series' bound does not know that l itself is
    rounded to a double (Erlang(3), exact, y = 1e-9: l = -41.35, k_hi = 2, the
    bound 4.0e-15, one ulp 7.1e-15; the error 0.9 times the bound, and 1.3
    times with the rates 1e-12 apart)"""
    b = 2.0 ** -53 * (n + 9) * (np.asarray(khi, np.float64) + 1) + 2.0 ** -56
    return b if l is None else b + np.spacing(np.abs(np.asarray(l, np.float64)))
