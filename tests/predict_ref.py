"""The tests' CPU restatement of include/pht_predict.h (tests/predict_spec.c,
compiled here with ``cc -O2 -ffp-contract=off`` into a shared object in a
temporary directory, as tests/loglik_unif_ref.py compiles its own) behind numpy
wrappers, the analytic moments the replicates are checked against, and the
tests' generators.  Shared by tests/test_predict.py and
tests/test_gpu_predict.py."""
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
_lp = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
_SPEC = None

KEY = (20260, 1019)  # the one key of every deterministic check
ALPHA = 1e-9         # Dvoretzky-Kiefer-Wolfowitz level


def spec():
    global _SPEC
    if _SPEC is None:
        td = tempfile.mkdtemp(prefix="pht_predict_spec_")
        atexit.register(shutil.rmtree, td, ignore_errors=True)
        so = os.path.join(td, "predict_spec.so")
        cc = shutil.which("cc") or shutil.which("gcc")
        subprocess.run([cc, "-O2", "-ffp-contract=off", "-shared", "-fPIC", f"-I{os.path.join(REPO, 'include')}",
                        "-o", so, os.path.join(HERE, "predict_spec.c"), "-lm"], check=True)
        L = C.CDLL(so)
        L.pspec_tab_words.argtypes = [C.c_int]
        L.pspec_flags.argtypes = [C.c_int, _dp, _dp]
        L.pspec_flags.restype = C.c_uint
        L.pspec_table.argtypes = [C.c_int, _dp, _dp, _dp]
        L.pspec_run.argtypes = [C.c_int, _dp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_long, C.c_uint32, C.c_double,
                                C.c_int, C.c_int, _dp, _dp, _ip, _lp, _lp, _dp, _dp]
        L.pspec_table.restype = L.pspec_run.restype = None
        _SPEC = L
    return _SPEC


def _flat(S, s):
    S = np.asarray(S, np.float64)
    return S.shape[0], np.ascontiguousarray(S.reshape(-1, order="F")), np.ascontiguousarray(s, np.float64).reshape(-1)


def table(S, s):
    """(flag, tab [n + n n]) of one draw (tab zero for a flagged draw)"""
    n, Sf, sf = _flat(S, s)
    tab = np.zeros(spec().pspec_tab_words(n))
    flag = int(spec().pspec_flags(n, Sf, sf))
    if flag == 0:
        spec().pspec_table(n, Sf, sf, tab)
    return flag, tab


def predict(S_list, s_list, nrep, key=KEY, rep0=0, draw0=0, edges=None, horizon=np.inf, max_jumps=1 << 20):
    """The restatement's Sweeper.predict(..., pointwise=True): the same dict
    (finalised by phasetype_amd.predict_finalise from the restatement's
    words), draw by draw."""
    import phasetype_amd as P

    edges = np.zeros(0) if edges is None else np.ascontiguousarray(edges, np.float64)
    nd, ne = len(S_list), len(edges)
    words, counts = np.zeros((nd, 8), np.int64), np.zeros((nd, ne + 1), np.int64)
    ymin, ymax = np.full(nd, np.inf), np.full(nd, -np.inf)
    y, nj = np.full((nd, nrep), np.nan), np.zeros((nd, nrep), np.int32)
    flags = np.zeros(nd, np.int32)
    for d, (S, s) in enumerate(zip(S_list, s_list)):
        flags[d], tab = table(S, s)
        if flags[d]:
            continue
        lo, hi = np.zeros(1), np.zeros(1)
        spec().pspec_run(np.asarray(S).shape[0], tab, key[0], key[1], rep0, nrep, draw0 + d, float(horizon),
                         int(max_jumps), ne, edges if ne else np.zeros(1), y[d], nj[d], words[d], counts[d], lo, hi)
        ymin[d], ymax[d] = lo[0], hi[0]
    out = P.predict_finalise(words, counts, ymin, ymax, flags, edges)
    out["y"], out["jumps"] = y, nj
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_same(a, b, pointwise=True):
    """two predict results agree bit for bit"""
    assert np.array_equal(a["flags"], b["flags"])
    assert np.array_equal(a["words"], b["words"]), (a["words"], b["words"])
    assert np.array_equal(a["counts"], b["counts"])
    assert np.array_equal(bits(a["ymin"]), bits(b["ymin"])) and np.array_equal(bits(a["ymax"]), bits(b["ymax"]))
    if pointwise:
        assert np.array_equal(bits(a["y"]), bits(b["y"]))
        assert np.array_equal(a["jumps"], b["jumps"])


# ---- generators -------------------------------------------------------------
def bd(n):
    from phasetype_amd.synth import bd_exit

    return bd_exit(n)


def ring(n, exit_div=1.0):
    """tests/loglik_unif_ref.py's ring(n) (bd_exit(n) plus a rate 1.5 from state
    n back to state 1: cyclic), its exit rates divided by exit_div with the
    diagonal adjusted"""
    if exit_div == 1.0:
        from loglik_unif_ref import ring as ring1

        return ring1(n)
    S, s = bd(n)
    S[n - 1, 0] += 1.5
    s = s / exit_div
    np.fill_diagonal(S, 0.0)
    np.fill_diagonal(S, -(S.sum(axis=1) + s))
    return S, s


def one_state(rate=1.7):
    return np.array([[-rate]]), np.array([rate])


# ---- analytic quantities (pi = e_1) ----------------------------------------
def moments(S):
    """(m1, m2) = (-e1' S^-1 1, 2 e1' S^-2 1)"""
    Si = np.linalg.inv(np.asarray(S, np.float64))
    one = np.ones(Si.shape[0])
    return float(-(Si @ one)[0]), float(2.0 * (Si @ (Si @ one))[0])


def jump_moments(S):
    """mean and variance of the number of jumps to absorption (the visits to
    transient states): Z = (I - P)^-1 over the transient jump chain,
    mean e1' Z 1, variance e1' (2 Z - I) Z 1 - mean^2"""
    S = np.asarray(S, np.float64)
    n = S.shape[0]
    Pm = S / (-np.diag(S))[:, None]
    np.fill_diagonal(Pm, 0.0)
    Z = np.linalg.inv(np.eye(n) - Pm)
    one = np.ones(n)
    m = float((Z @ one)[0])
    return m, float(((2.0 * Z - np.eye(n)) @ (Z @ one))[0] - m * m)


def cdf(S, t):
    """1 - e1' exp(S t) 1 at each t"""
    from scipy.linalg import expm

    S = np.asarray(S, np.float64)
    return np.array([1.0 - expm(S * float(v))[0].sum() for v in np.atleast_1d(t)])


def dkw(R, alpha=ALPHA):
    return float(np.sqrt(np.log(2.0 / alpha) / (2.0 * R)))


def words_from_y(y, jumps, horizon=np.inf):
    """the 8 words recomputed from pointwise values by the (H, F) rule"""
    y = np.asarray(y, np.float64)
    ok = ~np.isnan(y)
    w = np.zeros(8, np.int64)
    for col, v in ((0, y[ok]), (2, y[ok] * y[ok])):
        h = np.rint(v)
        w[col] = int(h.astype(np.int64).sum())
        w[col + 1] = int(np.rint((v - h) * 2.0 ** 32).astype(np.int64).sum())
    w[4], w[5] = int(ok.sum()), int((~ok).sum())
    w[6] = int((y[ok] == horizon).sum())
    w[7] = int(np.asarray(jumps)[ok].sum())
    return w
