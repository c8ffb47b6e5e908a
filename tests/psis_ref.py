"""The tests' CPU restatement of include/pht_psis.h (tests/psis_spec.c,
compiled here with ``cc -O2 -ffp-contract=off`` into a shared object in a
temporary directory) behind numpy wrappers.  Shared by tests/test_psis.py and
tests/test_gpu_psis.py."""
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

F_BAD, F_SHORT, F_CONST, F_FIT = 1, 2, 4, 8


def spec():
    global _SPEC
    if _SPEC is None:
        td = tempfile.mkdtemp(prefix="pht_psis_spec_")
        atexit.register(shutil.rmtree, td, ignore_errors=True)
        so = os.path.join(td, "psis_spec.so")
        cc = shutil.which("cc") or shutil.which("gcc")
        subprocess.run([cc, "-O2", "-ffp-contract=off", "-shared", "-fPIC", f"-I{os.path.join(REPO, 'include')}",
                        "-o", so, os.path.join(HERE, "psis_spec.c"), "-lm"], check=True)
        L = C.CDLL(so)
        L.spec_psis.argtypes = [C.c_int, C.c_long, _dp, _dp, _dp, _dp, _ip]
        L.spec_tail_len.argtypes = L.spec_grid.argtypes = [C.c_int]
        L.spec_log1p.argtypes = L.spec_expm1.argtypes = [C.c_double]
        L.spec_log1p.restype = L.spec_expm1.restype = C.c_double
        _SPEC = L
    return _SPEC


def tail_len(S: int) -> int:
    return spec().spec_tail_len(int(S))


def psis(l, usable=None) -> dict:
    """PSIS-LOO of l[draw, observation] over the rows ``usable`` marks
    (default: all): dict(elpd_i, khat, lppd_i, flags, n_draws_used)."""
    l = np.asarray(l, np.float64)
    if usable is not None:
        l = l[np.asarray(usable, bool)]
    l = np.ascontiguousarray(l)
    S, N = l.shape
    elpd, khat, lppd = np.zeros(N), np.zeros(N), np.zeros(N)
    flags = np.zeros(N, np.int32)
    if spec().spec_psis(S, N, l, elpd, khat, lppd, flags) != 0:
        raise ValueError(f"spec_psis refused S = {S}")
    return dict(elpd_i=elpd, khat=khat, lppd_i=lppd, flags=flags, n_draws_used=S)
