"""The tests' CPU restatement of include/pht_loglik.h (tests/loglik_spec.c,
compiled here with ``cc -O2 -ffp-contract=off`` into a shared object in a
temporary directory) behind numpy wrappers.  Shared by tests/test_loglik.py
and tests/test_gpu_loglik.py."""
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


def spec():
    global _SPEC
    if _SPEC is None:
        td = tempfile.mkdtemp(prefix="pht_loglik_spec_")
        atexit.register(shutil.rmtree, td, ignore_errors=True)
        so = os.path.join(td, "loglik_spec.so")
        cc = shutil.which("cc") or shutil.which("gcc")
        subprocess.run([cc, "-O2", "-ffp-contract=off", "-shared", "-fPIC", f"-I{os.path.join(REPO, 'include')}",
                        "-o", so, os.path.join(HERE, "loglik_spec.c"), "-lm"], check=True)
        L = C.CDLL(so)
        L.spec_pointwise.argtypes = [C.c_int, _dp, C.c_long, _dp, _ip, _dp]
        L.spec_totals.argtypes = [C.c_long, _dp, _lp]
        L.spec_waic.argtypes = [C.c_long, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _ip]
        L.spec_pointwise.restype = L.spec_totals.restype = L.spec_waic.restype = None
        _SPEC = L
    return _SPEC


def pointwise(blocks, y, cens):
    """l[draw, observation] from the draw blocks (uint8 [draws, bytes])."""
    y = np.ascontiguousarray(y, np.float64)
    cens = np.ascontiguousarray(cens, np.int32)
    blocks = np.ascontiguousarray(blocks, np.uint8)
    n = (blocks.shape[1] // 8 - 2) // 3
    out = np.zeros((blocks.shape[0], len(y)))
    for d in range(blocks.shape[0]):
        spec().spec_pointwise(n, blocks[d].view(np.float64), len(y), y, cens, out[d])
    return out


def totals(l):
    """int64 [draws, 4] words [H, F, nbad, nobs] from l[draw, observation] of
    usable draws (NaN = a bad observation; a flagged draw's words are all zero,
    which the caller sets)."""
    l = np.ascontiguousarray(l, np.float64)
    out = np.zeros((l.shape[0], 4), np.int64)
    for d in range(l.shape[0]):
        spec().spec_totals(l.shape[1], l[d], out[d])
    return out


def waic_state(l, state=None):
    """The WAIC accumulators after the draws of l[draw, observation], from
    ``state`` (default: reset)."""
    l = np.ascontiguousarray(l, np.float64)
    N = l.shape[1]
    st = ({k: np.zeros(N) for k in ("ref", "S1", "S2", "m", "r")} if state is None
          else {k: np.array(state[k], np.float64) for k in ("ref", "S1", "S2", "m", "r")})
    st["cnt"] = np.zeros(N, np.int32) if state is None else np.array(state["cnt"], np.int32)
    spec().spec_waic(N, l.shape[0], l, st["ref"], st["S1"], st["S2"], st["m"], st["r"], st["cnt"])
    return st


def scaled_draws(n, scales=(0.8, 0.9, 1.0, 1.1, 1.25)):
    """bd_exit(n) with every rate scaled: the tests' draws, as (S_list, s_list)."""
    from phasetype_amd.synth import bd_exit

    S, s = bd_exit(n)
    return [S * c for c in scales], [s * c for c in scales]
