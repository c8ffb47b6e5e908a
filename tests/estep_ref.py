"""The tests' CPU restatement of include/pht_estep.h (tests/estep_spec.c,
compiled here with ``cc -O2 -ffp-contract=off`` into a shared object in a
temporary directory; the draws' tables are tests/loglik_unif_ref.py's) behind
numpy wrappers, the header's error bound, and the high-precision reference
(mpmath, 50 digits, Van Loan block exponentials).  Shared by
tests/test_estep.py and tests/test_gpu_estep.py."""
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
_lp = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
_SPEC = None
ROWS = 2048


def spec():
    global _SPEC
    if _SPEC is None:
        td = tempfile.mkdtemp(prefix="pht_estep_spec_")
        atexit.register(shutil.rmtree, td, ignore_errors=True)
        so = os.path.join(td, "estep_spec.so")
        cc = shutil.which("cc") or shutil.which("gcc")
        subprocess.run([cc, "-O2", "-ffp-contract=off", "-shared", "-fPIC", f"-I{os.path.join(REPO, 'include')}",
                        "-o", so, os.path.join(HERE, "estep_spec.c"), "-lm"], check=True)
        L = C.CDLL(so)
        L.espec_yscale.argtypes = [C.c_double]
        L.espec_yscale.restype = C.c_double
        L.espec_hist.argtypes = [C.c_int, C.c_double, C.c_double, _dp, C.c_long, _dp, _ip, C.c_double, _lp, _lp, _dp,
                                 _ip, _ip]
        L.espec_hist.restype = None
        L.espec_contract.argtypes = [C.c_int, _dp, _dp, _lp, C.c_int, C.c_double, _dp, _dp, _dp, _dp]
        L.espec_contract.restype = C.c_uint
        assert L.espec_words() == 4 * ROWS
        _SPEC = L
    return _SPEC


def yscale_of(ymax):
    return float(spec().espec_yscale(float(ymax)))


def hist(S, s, y, cens, yscale=None, ymax=None):
    """One draw over the observations: dict(words int64 [2, 2048, 2], totals
    int64 [H, F, nbad, nobs], l, klo, khi per observation, flag, K, yscale);
    K from ymax (default: the largest y, as a context holding y)."""
    y = np.ascontiguousarray(y, np.float64)
    cens = np.ascontiguousarray(cens, np.int32)
    ymax = float(np.max(y)) if ymax is None else float(ymax)
    ys = yscale_of(ymax) if yscale is None else float(yscale)
    t = U.table(S, s, ymax)
    words, tot = np.zeros(4 * ROWS, np.int64), np.zeros(4, np.int64)
    l = np.full(len(y), np.nan)
    klo, khi = np.zeros(len(y), np.int32), np.zeros(len(y), np.int32)
    if t["flag"] == 0:
        spec().espec_hist(t["K"], t["mu"], t["abar"], np.ascontiguousarray(t["tab"].reshape(-1)), len(y), y, cens,
                          ys, words, tot, l, klo, khi)
    return dict(words=words.reshape(2, ROWS, 2), totals=tot, l=l, klo=klo, khi=khi, flag=t["flag"], K=t["K"],
                yscale=ys)


def contract(S, s, words, yscale, K=ROWS - 1):
    """dict(Z [n], N [n, n] from i to j, E [n], flag) from one draw's words"""
    S = np.asarray(S, np.float64)
    n = S.shape[0]
    Z, N, E, A = np.zeros(n), np.zeros(n * n), np.zeros(n), np.zeros(n)
    flag = spec().espec_contract(n, np.ascontiguousarray(S.reshape(-1, order="F")),
                                 np.ascontiguousarray(s, np.float64),
                                 np.ascontiguousarray(words, np.int64).reshape(-1), int(K), float(yscale), Z, N, E, A)
    return dict(Z=Z, N=N.reshape(n, n, order="F").copy(), E=E, A=A, flag=int(flag))


def estep(S, s, y, cens, yscale=None, ymax=None):
    """hist + contract of one draw, with ``loglik`` as the library reports it
    (H + F 2^-32; -inf with a bad observation, NaN for a flagged draw)"""
    h = hist(S, s, y, cens, yscale, ymax)
    c = contract(S, s, h["words"], h["yscale"])
    tot = h["totals"]
    ll = float(tot[0]) + float(tot[1]) * 2.0 ** -32
    ll = np.nan if h["flag"] else (-np.inf if tot[2] > 0 else ll)
    return dict(h, Z=c["Z"], N=c["N"], E=c["E"], A=c["A"], loglik=ll, nbad=int(tot[2]))


def bounds(n, y, cens, klo, khi, good, yscale):
    """the header's a-priori error bound for Z, N, E (scalars: it holds for
    every cell) over the good observations"""
    y, khi, klo = np.asarray(y, np.float64)[good], np.asarray(khi, np.float64)[good], np.asarray(klo, np.float64)[good]
    ex = np.asarray(cens)[good] == 0
    W = khi - klo + 1
    kmax = float(np.max(khi)) if len(khi) else 0.0
    rel = 4.0 * (n + 9) * (khi + 1) * 2.0 ** -53 + 2.0 ** -56

    def b(m, q):
        return float(np.sum(W * 2.0 ** -41 * q + rel * m) + 2.0 * (kmax + 1) * 2.0 ** -53 * np.sum(m))
    one = np.ones_like(y)
    return dict(Z=b(y, yscale * one), N=b(khi + 1, khi + 1),
                E=float(np.sum((W * 2.0 ** -41 + rel)[ex]) + 2.0 * (kmax + 1) * 2.0 ** -53 * np.sum(ex)),
                A=float(np.sum((W * 2.0 ** -41 + rel)[~ex]) + 2.0 * (kmax + 1) * 2.0 ** -53 * np.sum(~ex)))


def mp_reference(S, s, y, cens, dps=50):
    """Z, N, E (float64 of the 50-digit values) summed over the observations,
    and l per observation: per observation one Van Loan block exponential
    expm([[S, b pi], [0, S]] y), whose upper right block is
    M = int_0^y e^{S (y - u)} b pi e^{S u} du, M[j, i] = J_ij =
    int (pi e^{S u})_i (e^{S (y - u)} b)_j du (b = s exact, 1 censored): the
    time in i is J_ii / like, the jumps i -> j are S_ij J_ij / like."""
    import mpmath as mp

    S = np.asarray(S, np.float64)
    n = S.shape[0]
    with mp.workdps(dps):
        Z = [mp.mpf(0)] * n
        E = [mp.mpf(0)] * n
        A = [mp.mpf(0)] * n
        N = [[mp.mpf(0)] * n for _ in range(n)]
        ls = []
        for yv, cv in zip(y, cens):
            b = [mp.mpf(1) if cv else mp.mpf(float(s[i])) for i in range(n)]
            M = mp.zeros(2 * n)
            for i in range(n):
                for j in range(n):
                    M[i, j] = M[n + i, n + j] = mp.mpf(float(S[i, j]))
                M[i, n] = b[i]  # b pi, pi = e_1
            X = mp.expm(M * mp.mpf(float(yv)))
            like = sum(X[0, j] * b[j] for j in range(n))  # pi e^{S y} b
            ls.append(float(mp.log(like)))
            for i in range(n):
                Z[i] += X[i, n + i] / like
                if cv:
                    A[i] += X[0, i] / like
                else:
                    E[i] += X[0, i] * mp.mpf(float(s[i])) / like
                for j in range(n):
                    if i != j and S[i, j] != 0.0:
                        N[i][j] += mp.mpf(float(S[i, j])) * X[j, n + i] / like
        return dict(Z=np.array([float(v) for v in Z]), N=np.array([[float(v) for v in r] for r in N]),
                    E=np.array([float(v) for v in E]), A=np.array([float(v) for v in A]), l=np.array(ls))
