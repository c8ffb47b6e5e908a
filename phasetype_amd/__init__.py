"""phasetype_amd — MI355X-native PhaseType MCMC hot path.

Python mirror of the reference's R API over the C ABI of libPhaseType.so
(include/phasetype_amd.h):

* ``phtMCMC(x, states, beta, nu, zeta, n, mhit=1, ...)``   — R/phtMCMC.R:1-97
* ``phtMCMC2(x, TT, beta, nu, zeta, n, censored, C, method, mhit, ...)`` — R/phtMCMC2.R:1-86
* ``LJMA_Gibbs(...)`` — the 15-argument ``.C`` routine itself
  (src/PHT_MCMC_Aslett.c:104), as R's ``.C`` would call it.
* ``Sweeper`` — one GPU shard, one Gibbs step 1 per call (the seam of
  LJMA_MHsample_*; used by the parity tests and bench.py).

All compute runs in HIP kernels; there is no CPU fallback: without a GPU the
calls raise.  The library is loaded lazily so that importing works on a
CPU-only machine (the build check).
"""
from __future__ import annotations

import ctypes as C
import glob
import os

import numpy as np

from . import build as _build

__all__ = ["load", "LJMA_Gibbs", "phtMCMC", "phtMCMC2", "Sweeper", "gibbs_chains", "PhaseTypeError", "METHODS",
           "log_lik", "waic", "waic_from_state", "ph_curves", "loglik_block", "loglik_total", "theta_to_S",
           "EVALUATORS", "evaluator_runs", "pred_table", "predict_finalise", "predict_combine", "rph",
           "posterior_predictive", "ppc", "ppc_from_predict", "quantiles_from_counts", "loo", "loo_from_psis",
           "loo_compare", "PSIS_MAX_DRAWS", "estep_contract", "expected_stats", "complete_stats",
           "em_step", "ph_em", "ESTEP_MAX_OBS", "qph", "pph", "dph", "ph_quantiles", "quantile_host",
           "Q_F_P", "Q_F_T0", "Q_F_BEYOND", "Q_F_EVAL", "Q_F_CAP", "Q_F_DRAW",
           "fleet_forecast", "forecast_combine", "forecast_finalise", "forecast_host", "forecast_moments",
           "forecast_count_quantiles", "FORECAST_MAX_H", "FORECAST_MAX_UNITS",
           "fleet_condition", "condition_combine", "condition_finalise", "condition_host", "ph_state", "ph_mrl",
           "CONDITION_MAX_H", "CONDITION_MAX_UNITS", "CD_F_TRAP", "CD_F_HCAP",
           "fleet_spares", "spares_combine", "spares_finalise", "spares_host", "ph_renewal",
           "replace_host", "age_replacement", "ph_rmean", "ph_replacement", "fleet_replacement",
           "replacement_summary", "replacement_overdue", "REPLACE_MAX_AGES", "REPLACE_MAX_PAIRS",
           "RP_A_BEYOND", "RP_A_EVAL", "RP_A_DRAW", "RP_F_COST", "RP_F_DRAW", "RP_F_NOAGE", "RP_F_UNREFINED",
           "RP_F_EDGE", "RP_F_EVAL", "RP_F_NEVER", "RP_F_CAP"]

# R/phtMCMC2.R:66-70; "UNIF" (8) is not a reference method: the opt-in
# uniformisation sampler (phasetype_amd/csrc/pht_unif.h), lowest precedence
METHODS = {"MHRS": 1, "ECS": 2, "DCS": 4, "UNIF": 8}


class PhaseTypeError(RuntimeError):
    pass


_dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_ip = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_lp = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
_up = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
REDUCE_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_longlong), C.c_int, C.c_void_p)

_LIB = None

# every symbol include/phasetype_amd.h declares (tests check the exports)
EXPORTS = [
    "LJMA_Gibbs", "R_init_PhaseType", "pht_last_error", "pht_device_count", "pht_bind_lapack", "pht_set_seed",
    "pht_unif_rand", "pht_rgamma", "pht_in_R", "pht_set_verbose", "pht_zexp", "pht_params_bytes", "pht_stats_len",
    "pht_build_params", "pht_ctx_create", "pht_ctx_destroy", "pht_ctx_set_obs", "pht_ctx_sweep",
    "pht_ctx_sweep_debug", "pht_ctx_last_kernel_ms", "pht_ctx_flagged_obs", "pht_ctx_set_global_count", "pht_gibbs_run",
    "pht_gibbs_run_resident",
    "pht_gibbs_run_chains", "pht_rccl_unique_id", "pht_ctx_rccl_prepare", "pht_ctx_attach_rccl", "pht_ctx_rccl_allreduce",
    "pht_loglik_bytes", "pht_loglik_build", "pht_theta_to_S", "pht_ctx_loglik", "pht_ctx_loglik_reset",
    "pht_ctx_loglik_state", "pht_ctx_loglik_unif", "pht_ctx_loglik_unif_K",
    "pht_pred_words", "pht_pred_table_words", "pht_pred_build", "pht_ctx_predict",
    "pht_ctx_loo_begin", "pht_ctx_loo_fill", "pht_ctx_loo_fill_unif", "pht_ctx_loo", "pht_ctx_loo_end",
    "pht_estep_words", "pht_estep_yscale", "pht_ctx_estep", "pht_estep_contract", "pht_ctx_estep_grid_cap",
    "pht_ctx_estep_ms",
    "pht_ctx_quantile", "pht_ctx_quantile_ms", "pht_quantile_host",
    "pht_ctx_forecast", "pht_ctx_forecast_units", "pht_ctx_forecast_grid_cap", "pht_ctx_forecast_ms",
    "pht_forecast_host",
    "pht_ctx_condition", "pht_ctx_condition_grid_cap", "pht_ctx_condition_ms", "pht_condition_host",
    "pht_ctx_spares", "pht_ctx_spares_grid_cap", "pht_ctx_spares_ms", "pht_spares_host",
    "pht_ctx_replace", "pht_ctx_replace_ms", "pht_replace_host",
]


def lib_key() -> str:
    """Identity of the loaded native library, which bench.py keys its PMC
    counters on (counters measured on another build are not reported):
    "src:<sha256 of the build inputs>" for the in-tree library (the same for
    every build of those sources: the .so bytes embed the build directory),
    "file:<sha256 of the file>" for a PHT_LIB variant."""
    import hashlib

    path = load()._pht_path
    if os.path.abspath(path) == os.path.abspath(_build.LIB) and "PHT_LIB" not in os.environ:
        return "src:" + _build.source_key()
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 20), b""):
            h.update(chunk)
    return "file:" + h.hexdigest()


def _lapack_path():
    env = os.environ.get("PHT_LAPACK_LIB")
    if env:
        return env, os.environ.get("PHT_LAPACK_PREFIX", "")
    import scipy

    d = os.path.join(os.path.dirname(os.path.dirname(scipy.__file__)), "scipy.libs")
    cands = sorted(glob.glob(os.path.join(d, "libscipy_openblas-*.so")))
    if not cands:
        raise PhaseTypeError("no LP64 LAPACK found for the per-sweep eigendecomposition (set PHT_LAPACK_LIB)")
    return cands[0], "scipy_"


def load(build_if_needed: bool = True) -> C.CDLL:
    """Load (building first if stale) phasetype_amd/_lib/libPhaseType.so."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = os.environ.get("PHT_LIB")  # a variant build (tools/ab.py)
    if path is None:
        if build_if_needed and _build.needs_build():
            _build.build()
        path = _build.LIB
    if not os.path.exists(path):
        raise PhaseTypeError(f"native library missing: {path} (run phasetype_amd/build.py)")
    L = C.CDLL(path, mode=C.RTLD_LOCAL)
    L._pht_path = os.path.abspath(path)
    L.pht_last_error.restype = C.c_char_p
    L.pht_bind_lapack.argtypes = [C.c_char_p, C.c_char_p]
    L.pht_set_seed.argtypes = [C.c_uint32]
    L.pht_unif_rand.restype = C.c_double
    L.pht_rgamma.restype = C.c_double
    L.pht_rgamma.argtypes = [C.c_double, C.c_double]
    L.pht_zexp.argtypes = [_dp, C.c_long]
    L.pht_build_params.argtypes = [C.c_int, _dp, _dp, C.c_int, C.c_void_p, C.c_int]
    L.pht_ctx_create.restype = C.c_void_p
    L.pht_ctx_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.pht_ctx_destroy.argtypes = [C.c_void_p]
    L.pht_ctx_set_obs.argtypes = [C.c_void_p, _dp, _ip, C.c_long, C.c_long]
    L.pht_ctx_sweep.argtypes = [C.c_void_p, _dp, _dp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _lp]
    L.pht_ctx_sweep_debug.argtypes = [C.c_void_p, _dp, _dp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _lp,
                                      _ip, _ip, _ip, _up, _lp, _ip]
    L.pht_ctx_last_kernel_ms.restype = C.c_float
    L.pht_ctx_last_kernel_ms.argtypes = [C.c_void_p]
    L.pht_ctx_flagged_obs.restype = C.c_longlong
    L.pht_ctx_flagged_obs.argtypes = [C.c_void_p]
    L.pht_ctx_set_global_count.argtypes = [C.c_void_p, C.c_longlong]
    L.pht_gibbs_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, _ip, _dp, C.c_int, C.c_int,
                                _dp, _dp, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    L.pht_gibbs_run_resident.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp, _ip, _dp, C.c_int, _dp,
                                         _dp, C.POINTER(C.c_double)]
    L.pht_gibbs_run_chains.argtypes = [C.POINTER(C.c_void_p), C.c_int, _up, C.c_int, C.c_int, C.c_int, _dp, _dp,
                                       _ip, _dp, C.c_int, _dp, _dp, C.POINTER(C.c_double)]
    L.pht_rccl_unique_id.argtypes = [C.c_void_p]
    L.pht_ctx_rccl_prepare.argtypes = [C.c_void_p, C.c_int]
    L.pht_ctx_attach_rccl.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
    L.pht_ctx_rccl_allreduce.argtypes = [C.c_void_p, _lp, C.c_int]
    L.LJMA_Gibbs.argtypes = [_ip, _ip, _ip, _ip, _ip, _dp, _dp, _ip, _dp, _dp, _ip, _ip, _dp, _ip, _dp]
    L.pht_loglik_bytes.argtypes = [C.c_int]
    L.pht_loglik_build.argtypes = [C.c_int, _dp, _dp, C.c_void_p, C.c_int]
    L.pht_theta_to_S.argtypes = [C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp]
    L.pht_ctx_loglik.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, _lp, C.c_void_p, C.c_int]
    L.pht_ctx_loglik_reset.argtypes = [C.c_void_p]
    L.pht_ctx_loglik_state.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, _dp, _ip]
    L.pht_ctx_loglik_unif.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_int, _lp, C.c_void_p, C.c_int, _ip]
    L.pht_ctx_loglik_unif_K.argtypes = [C.c_void_p, C.c_double]
    L.pht_pred_table_words.argtypes = [C.c_int]
    L.pht_pred_build.argtypes = [C.c_int, _dp, _dp, _dp, C.c_int]
    L.pht_ctx_predict.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_int, C.c_longlong, C.c_uint32, C.c_uint32,
                                  C.c_uint32, C.c_double, C.c_int, C.c_int, _dp, C.c_int, _lp, _lp, _dp, _dp,
                                  C.c_void_p, C.c_void_p, _ip]
    L.pht_ctx_loo_begin.argtypes = [C.c_void_p, C.c_int]
    L.pht_ctx_loo_fill.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, _lp]
    L.pht_ctx_loo_fill_unif.argtypes = [C.c_void_p, C.c_int, C.c_int, _dp, _dp, C.c_int, _lp, _ip]
    L.pht_ctx_loo.argtypes = [C.c_void_p, _dp, _dp, _dp, _ip, C.POINTER(C.c_int)]
    L.pht_ctx_loo_end.argtypes = [C.c_void_p]
    L.pht_estep_yscale.restype = C.c_double
    L.pht_estep_yscale.argtypes = [C.c_double]
    L.pht_ctx_estep.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_int, C.c_double, _lp, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, _ip]
    L.pht_estep_contract.argtypes = [C.c_int, _dp, _dp, _lp, C.c_int, C.c_double, _dp, _dp, _dp, _dp]
    L.pht_ctx_estep_grid_cap.argtypes = [C.c_void_p, C.c_int]
    L.pht_ctx_estep_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.pht_ctx_quantile.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_int, _dp, C.c_double, C.c_double, C.c_int, _dp,
                                   _dp, _dp, _ip, _up, _ip]
    L.pht_ctx_quantile_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.pht_quantile_host.argtypes = [C.c_int, _dp, _dp, C.c_int, _dp, C.c_double, C.c_double, _dp, _dp, _dp, _ip, _up]
    L.pht_ctx_forecast.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_int, _dp, C.c_int, _lp, C.c_void_p, C.c_void_p,
                                   C.c_void_p, _ip]
    L.pht_ctx_forecast_units.restype = C.c_long
    L.pht_ctx_forecast_units.argtypes = [C.c_void_p, C.c_void_p]
    L.pht_ctx_forecast_grid_cap.argtypes = [C.c_void_p, C.c_int]
    L.pht_ctx_forecast_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.pht_forecast_host.argtypes = [C.c_int, _dp, _dp, C.c_long, _dp, C.c_int, _dp, C.c_double, _lp, C.c_void_p,
                                    C.c_void_p, C.c_void_p]
    L.pht_ctx_condition.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_int, _dp, C.c_int, _lp, _dp] + \
        [C.c_void_p] * 7 + [_ip]
    L.pht_ctx_condition_grid_cap.argtypes = [C.c_void_p, C.c_int]
    L.pht_ctx_condition_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.pht_condition_host.argtypes = [C.c_int, _dp, _dp, C.c_long, _dp, C.c_int, _dp, C.c_double, _lp, _dp] + \
        [C.c_void_p] * 7
    L.pht_ctx_spares.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_int, _dp, C.c_int, _lp, _dp] + \
        [C.c_void_p] * 6 + [_ip]
    L.pht_ctx_spares_grid_cap.argtypes = [C.c_void_p, C.c_int]
    L.pht_ctx_spares_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.pht_spares_host.argtypes = [C.c_int, _dp, _dp, C.c_long, _dp, C.c_int, _dp, C.c_double, _lp, _dp] + \
        [C.c_void_p] * 6
    L.pht_ctx_replace.argtypes = [C.c_void_p, C.c_int, _dp, _dp, C.c_int, _dp, C.c_int, _dp, _dp, C.c_int, _dp, _dp,
                                  _dp, _dp, _ip, _ip, _up, _dp, _ip] + [C.c_void_p] * 4
    L.pht_ctx_replace_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.pht_replace_host.argtypes = [C.c_int, _dp, _dp, C.c_int, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _ip, _ip,
                                   _up, _dp, _dp, _dp, _dp, _up]
    p, pre = _lapack_path()
    if L.pht_bind_lapack(p.encode(), pre.encode()) != 0:
        raise PhaseTypeError(L.pht_last_error().decode())
    _LIB = L
    return L


def _err(L) -> PhaseTypeError:
    return PhaseTypeError(L.pht_last_error().decode() or "unknown error")


def _pack_draws(S_list, s_list, n: int):
    """(S_all [draws, n n] column-major, s_all [draws, n], draws) of draws (S, s)."""
    S_all = np.ascontiguousarray([np.asarray(S, np.float64).reshape(-1, order="F") for S in S_list])
    s_all = np.ascontiguousarray([np.asarray(s, np.float64).reshape(-1) for s in s_list])
    nd = S_all.shape[0]
    if nd < 1 or S_all.shape != (nd, n * n) or s_all.shape != (nd, n):
        raise ValueError(f"need at least one draw, each S [{n}, {n}] and s [{n}]")
    return S_all, s_all, nd


def _totals_dict(tot, bad_draw, **more) -> dict:
    """loglik_blocks' dict from the int64 totals [draws, 4] = [H, F, nbad, nobs]."""
    tot = tot.reshape(-1, 4)
    out = dict(H=tot[:, 0].copy(), F=tot[:, 1].copy(), nbad=tot[:, 2].copy(), nobs=tot[:, 3].copy(),
               bad_draw=bad_draw, **more)
    out["total"] = loglik_total(out["H"], out["F"], out["nbad"], bad_draw)
    return out


def _ms_pair(read, ctx) -> tuple:
    """The two device times of a pht_ctx_X_ms entry point."""
    a, b = C.c_float(0), C.c_float(0)
    read(ctx, C.byref(a), C.byref(b))
    return (a.value, b.value)


def set_seed(seed: int) -> None:
    """R's set.seed() for the standalone host stream (inside R, R's own)."""
    load().pht_set_seed(int(seed) & 0xFFFFFFFF)


def device_count() -> int:
    return load().pht_device_count()


def zexp_for(y) -> int:
    y = np.ascontiguousarray(y, np.float64)
    return load().pht_zexp(y, len(y))


def stats_len(n: int) -> int:
    return 2 * n + n * n + 16


# extra-word indices (phasetype_amd/csrc/pht_layout.h): the ECS exact
# kernels' DEBUG launches count general-ARMS and private-envelope rounds there
XDBG_GENERAL, XDBG_PRIVATE = 8, 9


def split_stats(st, n):
    """int64 block -> (zq[n], B[n], N[n,n] as N[from, to], extras[16])."""
    st = np.asarray(st)
    zq = st[:n]
    B = st[n:2 * n]
    N = st[2 * n:2 * n + n * n].reshape(n, n).T  # N[i + j n] -> [i, j]
    return zq, B, N, st[2 * n + n * n:]


RCCL_ID_BYTES = 128


def rccl_unique_id() -> bytes:
    """A fresh RCCL unique id (one rank creates it and broadcasts it)."""
    L = load()
    buf = C.create_string_buffer(RCCL_ID_BYTES)
    if L.pht_rccl_unique_id(buf) != 0:
        raise _err(L)
    return buf.raw


class Sweeper:
    """One GPU shard of observations; one Gibbs step 1 per ``sweep`` call."""

    def __init__(self, n: int, method: int, mhit: int = 1, device: int = 0):
        self.L = load()
        self.n = n
        self.ctx = self.L.pht_ctx_create(device, n, method, mhit)
        if not self.ctx:
            raise _err(self.L)
        self.count = 0
        self.ymax = 0.0  # the largest observation (estep's default yscale)
        self.flagged_obs = 0  # flagged observation-sweeps of the last gibbs() (pht_ctx_flagged_obs)

    def set_obs(self, y, censored=None, obs0: int = 0):
        y = np.ascontiguousarray(y, np.float64)
        cen = np.zeros(len(y), np.int32) if censored is None else np.ascontiguousarray(censored, np.int32)
        if self.L.pht_ctx_set_obs(self.ctx, y, cen, len(y), obs0) != 0:
            raise _err(self.L)
        self.count = len(y)
        self.ymax = float(np.max(y)) if len(y) else 0.0

    def sweep(self, S, s, key=(1, 2), sweep: int = 1, zexp: int = 40):
        out = np.zeros(stats_len(self.n), np.int64)
        Sf = np.ascontiguousarray(np.asarray(S, np.float64).reshape(-1, order="F"))
        if self.L.pht_ctx_sweep(self.ctx, Sf, np.ascontiguousarray(s, np.float64), key[0], key[1], sweep, zexp,
                                out) != 0:
            raise _err(self.L)
        return out

    def sweep_debug(self, S, s, key=(1, 2), sweep: int = 1, zexp: int = 40):
        n, l = self.n, self.count
        out = np.zeros(stats_len(n), np.int64)
        B, pre, fl = np.zeros(l, np.int32), np.zeros(l, np.int32), np.zeros(l, np.int32)
        nd = np.zeros(l, np.uint32)
        zq = np.zeros(l * n, np.int64)
        N = np.zeros(l * n * n, np.int32)
        Sf = np.ascontiguousarray(np.asarray(S, np.float64).reshape(-1, order="F"))
        if self.L.pht_ctx_sweep_debug(self.ctx, Sf, np.ascontiguousarray(s, np.float64), key[0], key[1], sweep,
                                      zexp, out, B, pre, fl, nd, zq, N) != 0:
            raise _err(self.L)
        return dict(stats=out, B=B, pre=pre, flags=fl, ndraw=nd, zq=zq.reshape(l, n),
                    N=N.reshape(l, n, n).transpose(0, 2, 1))

    def set_global_count(self, total: int) -> None:
        """Observations over all shards of a multi-process run: every sweep of
        gibbs() then checks the reduced statistics account for exactly that
        many (pht_ctx_set_global_count)."""
        if self.L.pht_ctx_set_global_count(self.ctx, int(total)) != 0:
            raise _err(self.L)

    def rccl_prepare(self, max_len: int = 256) -> None:
        """Local preconditions of attach_rccl / rccl_allreduce (RCCL loadable,
        no communicator yet, device, a staging buffer of max_len words):
        pht_ctx_rccl_prepare.  Ranks agree on it before anyone attaches."""
        if self.L.pht_ctx_rccl_prepare(self.ctx, int(max_len)) != 0:
            raise _err(self.L)

    def attach_rccl(self, uid: bytes, nranks: int, rank: int) -> None:
        """Sum every sweep's statistics block over ``nranks`` processes with
        an RCCL all-reduce on this shard's stream (pht_ctx_attach_rccl, the
        collective ncclCommInitRank); ``uid`` = rccl_unique_id() of one rank,
        the same on all, after rccl_prepare() on every rank.  gibbs() then
        needs no ``reduce``."""
        if len(uid) != RCCL_ID_BYTES:
            raise ValueError(f"RCCL unique id must be {RCCL_ID_BYTES} bytes, got {len(uid)}")
        if self.L.pht_ctx_attach_rccl(self.ctx, uid, nranks, rank) != 0:
            raise _err(self.L)

    def rccl_allreduce(self, buf: np.ndarray) -> None:
        """In-place sum of an int64 vector over the attached communicator
        (the same all-reduce a sweep runs on its statistics block)."""
        if buf.dtype != np.int64 or not buf.flags.c_contiguous:
            raise ValueError("rccl_allreduce needs a contiguous int64 array")
        if self.L.pht_ctx_rccl_allreduce(self.ctx, buf, len(buf)) != 0:
            raise _err(self.L)

    def last_kernel_ms(self) -> float:
        return self.L.pht_ctx_last_kernel_ms(self.ctx)

    def gibbs(self, it, method, nu, zeta, T, C_, zexp, start=None, reduce=None, silent=True):
        """Gibbs loop over this shard; ``reduce(stats: np.ndarray) -> None``
        sums the int64 block across shards in place (multi-process)."""
        m = len(nu)
        res = np.zeros(it * m, np.float64)
        start = np.array([-1.0]) if start is None else np.ascontiguousarray(start, np.float64)
        cb = None
        if reduce is not None:
            def _cb(ptr, ln, user):
                try:
                    arr = np.ctypeslib.as_array(ptr, shape=(ln,))
                    reduce(arr)
                    return 0
                except Exception:  # noqa: BLE001 - reported through the C status
                    return 1
            cb = REDUCE_FN(_cb)
        kms = C.c_double(0.0)
        Tf = np.ascontiguousarray(np.asarray(T).reshape(-1, order="F"), np.int32)
        Cf = np.ascontiguousarray(np.asarray(C_, np.float64).reshape(-1, order="F"))
        rc = self.L.pht_gibbs_run(self.ctx, it, method, m, np.ascontiguousarray(nu, np.float64),
                                  np.ascontiguousarray(zeta, np.float64), Tf, Cf, zexp, int(silent), start, res,
                                  C.cast(cb, C.c_void_p) if cb else None, None, C.byref(kms))
        if rc != 0:
            raise _err(self.L)
        self.kernel_ms_total = kms.value
        self.flagged_obs = int(self.L.pht_ctx_flagged_obs(self.ctx))
        return res.reshape(m, it).T.copy()

    def gibbs_resident(self, it, method, nu, zeta, T, C_, zexp, start=None):
        """The device-resident chain (pht_gibbs_run_resident; opt-in,
        non-parity: Gamma draws from the device's counter-based sampler):
        every sweep and conjugate update runs on the GPU, one host wait."""
        m = len(nu)
        res = np.zeros(it * m, np.float64)
        start = np.array([-1.0]) if start is None else np.ascontiguousarray(start, np.float64)
        kms = C.c_double(0.0)
        Tf = np.ascontiguousarray(np.asarray(T).reshape(-1, order="F"), np.int32)
        Cf = np.ascontiguousarray(np.asarray(C_, np.float64).reshape(-1, order="F"))
        if self.L.pht_gibbs_run_resident(self.ctx, it, method, m, np.ascontiguousarray(nu, np.float64),
                                         np.ascontiguousarray(zeta, np.float64), Tf, Cf, zexp, start, res,
                                         C.byref(kms)) != 0:
            raise _err(self.L)
        self.kernel_ms_total = kms.value
        self.flagged_obs = int(self.L.pht_ctx_flagged_obs(self.ctx))
        return res.reshape(m, it).T.copy()

    def loglik_blocks(self, blocks, batch: int = 64, pointwise: bool = False, accumulate: bool = False):
        """pht_ctx_loglik on per-draw blocks (``loglik_block``; uint8
        [draws, pht_loglik_bytes(n)]) over this shard's observations.

        Returns ``H, F, nbad, nobs`` (int64 per draw), ``bad_draw`` (the
        draw's flag word is non-zero: a complex spectrum, a failed LAPACK call,
        a non-finite generator, or coefficients that cancel past the guard of
        include/pht_loglik.h, LL_F_ILLCOND, as a defective or nearly defective
        spectrum gives; never evaluated), ``nbad`` counts the observations
        that are bad for a usable draw (no density, or a sum that cancels
        past the guard), ``total`` (``loglik_total`` of this shard's words) and,
        with ``pointwise``, l[draw, observation] in the caller's order.
        ``accumulate`` feeds the per-observation WAIC state (waic_state).

        The words are exact integer sums, so shards and ranks add::

            w = np.stack([r["H"], r["F"], r["nbad"], r["nobs"]])
            reduce(w)                      # the int64 sum gibbs() is given
            total = loglik_total(w[0], w[1], w[2], r["bad_draw"])
        """
        blocks = np.ascontiguousarray(blocks, np.uint8)
        nb = self.L.pht_loglik_bytes(self.n)
        if blocks.ndim != 2 or blocks.shape[1] != nb:
            raise ValueError(f"blocks must be [draws, {nb}] bytes for n = {self.n}")
        nd = blocks.shape[0]
        tot = np.zeros(4 * nd, np.int64)
        pw = np.full((nd, self.count), np.nan) if pointwise else None
        if self.L.pht_ctx_loglik(self.ctx, nd, blocks.ctypes.data, int(batch), tot,
                                 pw.ctypes.data if pointwise else None, int(bool(accumulate))) != 0:
            raise _err(self.L)
        out = _totals_dict(tot, blocks[:, :8].copy().view(np.uint64).reshape(nd) != 0)
        if pointwise:
            out["pointwise"] = pw
        return out

    def loglik_unif(self, S_list, s_list, batch: int = 64, pointwise: bool = False, accumulate: bool = False):
        """pht_ctx_loglik_unif: the log-likelihood of each draw (S, s) over
        this shard by uniformisation (include/pht_loglik_unif.h): any finite
        generator, complex and defective spectra included, no LAPACK.

        The result is ``loglik_blocks``'s dict; ``bad_draw`` marks a draw with
        a non-finite entry or without a positive finite rate, ``flags`` holds
        the flag words.  An observation beyond the table (mu y above roughly
        1500) or below 2^-900 is bad for that draw (``nbad``, total -inf).
        ``accumulate`` continues the same WAIC state as ``loglik_blocks``."""
        S_all, s_all, nd = _pack_draws(S_list, s_list, self.n)
        tot = np.zeros(4 * nd, np.int64)
        flags = np.zeros(nd, np.int32)
        pw = np.full((nd, self.count), np.nan) if pointwise else None
        if self.L.pht_ctx_loglik_unif(self.ctx, nd, S_all.reshape(-1), s_all.reshape(-1), int(batch), tot,
                                      pw.ctypes.data if pointwise else None, int(bool(accumulate)), flags) != 0:
            raise _err(self.L)
        out = _totals_dict(tot, flags != 0, flags=flags)
        if pointwise:
            out["pointwise"] = pw
        return out

    def loglik_unif_K(self, mu: float) -> int:
        """The last table row K this context's observations give a draw with
        largest rate ``mu`` (pht_ctx_loglik_unif_K; at most 2047)."""
        K = self.L.pht_ctx_loglik_unif_K(self.ctx, float(mu))
        if K < 0:
            raise _err(self.L)
        return K

    def loglik(self, S_list, s_list, batch: int = 64, pointwise: bool = False, accumulate: bool = False,
               evaluator: str = "spectral", blocks=None):
        """Observed-data log-likelihood of each draw (S, s) over this shard:
        sum of log f(y) over exact and log Fbar(y) over censored observations;
        see loglik_blocks for the result, which gains ``evaluator``: per draw,
        "spectral" or "unif".

        ``evaluator``: "spectral" (the default; include/pht_loglik.h: a
        flagged draw is NaN: a complex spectrum, or a defective or nearly
        defective one whose coefficients cancel; an observation whose sum
        cancels past the guard is bad, so the draw's total is -inf), "unif"
        (every draw by uniformisation, include/pht_loglik_unif.h) or "auto"
        (spectral where the draw's block is usable and no observation is bad,
        uniformisation otherwise, NaN only for a non-finite generator).
        "auto" first runs the usable blocks totals-only to find the draws with
        bad observations, then issues one call per maximal run of draws of one
        evaluator, in draw order, so the WAIC state sees each draw once and
        in order.
        ``blocks``: the draws' spectral blocks where the caller has them."""
        if evaluator not in EVALUATORS:
            raise ValueError(f"evaluator must be one of {EVALUATORS}, got {evaluator!r}")
        S_list, s_list = list(S_list), list(s_list)
        kw = dict(batch=batch, pointwise=pointwise, accumulate=accumulate)
        if evaluator == "unif":
            out = self.loglik_unif(S_list, s_list, **kw)
            out["evaluator"] = np.full(len(S_list), "unif")
            return out
        if blocks is None:
            blocks = np.stack([loglik_block(S, s) for S, s in zip(S_list, s_list)])
        if evaluator == "spectral":
            out = self.loglik_blocks(blocks, **kw)
            out["evaluator"] = np.full(len(S_list), "spectral")
            return out
        parts = []
        for lo, hi, unif in self._auto_runs(blocks, batch):
            r = (self.loglik_unif(S_list[lo:hi], s_list[lo:hi], **kw) if unif
                 else self.loglik_blocks(blocks[lo:hi], **kw))
            r.pop("flags", None)
            r["evaluator"] = np.full(hi - lo, "unif" if unif else "spectral")
            parts.append(r)
        return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}

    def _auto_runs(self, blocks, batch: int = 64) -> list:
        """evaluator_runs for evaluator="auto": a totals-only spectral pass
        over the draws with a usable block (no WAIC accumulation, no pointwise
        rows) finds those with bad observations; they go to uniformisation
        with the flagged ones."""
        flags = np.ascontiguousarray(blocks[:, :8]).view(np.uint64).reshape(-1)
        nbad = np.zeros(len(flags), np.int64)
        usable = np.flatnonzero(flags == 0)
        if len(usable):
            nbad[usable] = self.loglik_blocks(blocks[usable], batch=batch)["nbad"]
        return evaluator_runs(flags, nbad)

    def estep(self, S_list, s_list, batch: int = 64, yscale=None, contract: bool = True, grid_cap: int = 0):
        """pht_ctx_estep: the expected sufficient statistics of each draw
        (S, s) given this shard's observations (include/pht_estep.h), by the
        uniformisation of ``loglik_unif`` (its limits apply).

        Returns ``Z`` [draws, n] (expected time in each state), ``N`` [draws,
        n, n] (expected transitions, N[d, i, j] from i to j, diagonal 0),
        ``E`` [draws, n] (expected exits), all on [0, y] and summed over the
        shard's good observations, ``A`` [draws, n] (the expected number of
        censored observations in each state at their censoring time; see
        ``complete_stats``), all None without ``contract``; ``loglik`` (-inf where an
        observation was bad, NaN for a flagged draw), ``H, F, nbad, nobs`` (the
        words of ``loglik_unif``, bit for bit), ``flags``, ``words`` (int64
        [draws, 2, 2048, 2] = [class, k, (G, T)]) and ``yscale``.

        The words are exact integer sums: shards and ranks that share one
        ``yscale`` (a power of two >= every observation anywhere; default:
        the smallest for this shard) add their words, then
        ``estep_contract(S, s, words, yscale)`` gives the statistics of the
        whole.  ``grid_cap``: most blocks of the histogram kernel (0: the
        default); the result does not depend on it.  ``last_estep_ms`` then
        holds the device time of the histograms and of the contraction."""
        n = self.n
        S_all, s_all, nd = _pack_draws(S_list, s_list, n)
        ys = float(self.L.pht_estep_yscale(self.ymax)) if yscale is None else float(yscale)
        nw = self.L.pht_estep_words()
        tot = np.zeros(4 * nd, np.int64)
        words = np.zeros((nd, nw), np.int64)
        flags = np.zeros(nd, np.int32)
        Z, N, E, A = ((np.zeros((nd, n)), np.zeros((nd, n * n)), np.zeros((nd, n)), np.zeros((nd, n))) if contract
                      else (None, None, None, None))
        if self.L.pht_ctx_estep_grid_cap(self.ctx, int(grid_cap)) != 0:
            raise _err(self.L)
        ptr = (lambda a: a.ctypes.data) if contract else (lambda a: None)
        if self.L.pht_ctx_estep(self.ctx, nd, S_all.reshape(-1), s_all.reshape(-1), int(batch), ys, tot,
                                words.ctypes.data, ptr(Z), ptr(N), ptr(E), ptr(A), flags) != 0:
            raise _err(self.L)
        self.last_estep_ms = _ms_pair(self.L.pht_ctx_estep_ms, self.ctx)
        tot = tot.reshape(nd, 4)
        out = dict(Z=Z, N=None if N is None else N.reshape(nd, n, n).transpose(0, 2, 1).copy(), E=E, A=A,
                   H=tot[:, 0].copy(), F=tot[:, 1].copy(), nbad=tot[:, 2].copy(), nobs=tot[:, 3].copy(), flags=flags,
                   words=words.reshape(nd, 2, nw // 4, 2), yscale=ys)
        out["loglik"] = loglik_total(out["H"], out["F"], out["nbad"], flags != 0)
        return out

    def quantile(self, S_list, s_list, probs, given: float = 0.0, tmax=None, batch: int = 64):
        """pht_ctx_quantile: for each draw (S, s) and each probability p the
        time t with P(T <= t | T > given) = p (include/pht_quantile.h), by a
        safeguarded Newton iteration on the uniformisation evaluator's log
        survival function; no observations are needed.

        Returns ``t`` (the quantile; with ``given`` > 0 the residual life
        t - given), ``lo`` and ``hi`` (the final bracket, absolute times),
        ``nev`` (evaluations per root) and ``flags`` (Q_F_* bits), each
        [draws, P] in the order of ``probs`` (any order, duplicates allowed),
        and ``bad_draw`` / ``draw_flags`` per draw as ``loglik_unif`` gives
        them.  p = 0 gives 0, p = 1 inf; a root beyond the horizon (``tmax``,
        default and at most 1400 / the largest rate) is inf with Q_F_BEYOND;
        any other flag is NaN.  ``last_quantile_ms`` then holds the device
        time of the table kernel and of the searches."""
        S_all, s_all, nd = _pack_draws(S_list, s_list, self.n)
        probs =np.ascontiguousarray(np.atleast_1d(probs), np.float64).reshape(-1)
        P_ = len(probs)
        if P_ < 1:
            raise ValueError("need at least one probability")
        t, lo, hi = np.zeros((nd, P_)), np.zeros((nd, P_)), np.zeros((nd, P_))
        nev, flags = np.zeros((nd, P_), np.int32), np.zeros((nd, P_), np.uint32)
        dflags = np.zeros(nd, np.int32)
        if self.L.pht_ctx_quantile(self.ctx, nd, S_all.reshape(-1), s_all.reshape(-1), P_, probs, float(given),
                                   np.inf if tmax is None else float(tmax), int(batch), t.reshape(-1), lo.reshape(-1),
                                   hi.reshape(-1), nev.reshape(-1), flags.reshape(-1), dflags) != 0:
            raise _err(self.L)
        self.last_quantile_ms = _ms_pair(self.L.pht_ctx_quantile_ms, self.ctx)
        return dict(t=t, lo=lo, hi=hi, nev=nev, flags=flags, bad_draw=dflags != 0, draw_flags=dflags)

    def replace(self, S_list, s_list, ages, cp, cf, batch: int = 64, pointwise: bool = False):
        """pht_ctx_replace: age-replacement policies (include/pht_replace.h).  A
        unit is replaced at failure (cost ``cf``) or at age tau (cost ``cp`` <
        ``cf``); for each draw (S, s) and each pair the age that minimises the
        long-run cost rate g(tau) = (cp + (cf - cp) F(tau)) / M(tau): the
        argmin over ``ages`` (1 .. 1024, positive, strictly increasing),
        refined by a 64-way multisection on the sign of g'.  No observations
        are needed.

        Returns ``t`` (the optimal age; inf with RP_F_NEVER where running to
        failure costs no more), ``g`` (its cost rate), ``lo`` and ``hi`` (the
        final bracket), ``j`` (the grid's argmin), ``nev`` (points evaluated)
        and ``flags`` (RP_F_* bits), each [draws, P]; ``m`` (the mean life),
        ``bad_draw`` and ``draw_flags`` per draw; with ``pointwise`` the curve
        ``lS`` = log Fbar, ``lf`` = log f, ``M`` (the restricted mean life) and
        ``age_flags`` (RP_A_* bits; a flagged age is NaN), each [draws, G].
        ``last_replace_ms`` then holds the device time of the tables with the
        curve and of the policies."""
        S_all, s_all, nd = _pack_draws(S_list, s_list, self.n)
        ages = np.ascontiguousarray(np.atleast_1d(ages), np.float64).reshape(-1)
        cp = np.ascontiguousarray(np.atleast_1d(cp), np.float64).reshape(-1)
        cf = np.ascontiguousarray(np.atleast_1d(cf), np.float64).reshape(-1)
        if len(cp) != len(cf):
            raise ValueError("cp and cf must have the same length")
        G, P_ = len(ages), len(cp)
        out = dict(t=np.zeros((nd, P_)), g=np.zeros((nd, P_)), lo=np.zeros((nd, P_)), hi=np.zeros((nd, P_)),
                   j=np.zeros((nd, P_), np.int32), nev=np.zeros((nd, P_), np.int32),
                   flags=np.zeros((nd, P_), np.uint32), m=np.zeros(nd))
        dflags = np.zeros(nd, np.int32)
        pw = [None] * 4
        if pointwise:
            out.update(lS=np.zeros((nd, G)), lf=np.zeros((nd, G)), M=np.zeros((nd, G)),
                       age_flags=np.zeros((nd, G), np.uint32))
            pw = [out[k].ctypes.data_as(C.c_void_p) for k in ("lS", "lf", "M", "age_flags")]
        if self.L.pht_ctx_replace(self.ctx, nd, S_all.reshape(-1), s_all.reshape(-1), G, ages, P_, cp, cf, int(batch),
                                  out["t"].reshape(-1), out["g"].reshape(-1), out["lo"].reshape(-1),
                                  out["hi"].reshape(-1), out["j"].reshape(-1), out["nev"].reshape(-1),
                                  out["flags"].reshape(-1), out["m"], dflags, *pw) != 0:
            raise _err(self.L)
        self.last_replace_ms = _ms_pair(self.L.pht_ctx_replace_ms, self.ctx)
        out.update(bad_draw=dflags != 0, draw_flags=dflags)
        return out

    def forecast_units(self) -> np.ndarray:
        """pht_ctx_forecast_units: the indices, in the order given to
        ``set_obs``, of this shard's censored observations (the units still in
        service); ``forecast``'s per-unit rows are in this order."""
        nc = self.L.pht_ctx_forecast_units(self.ctx, None)
        if nc < 0:
            raise _err(self.L)
        idx = np.zeros(nc, np.int64)
        if nc and self.L.pht_ctx_forecast_units(self.ctx, idx.ctypes.data) < 0:
            raise _err(self.L)
        return idx

    def forecast(self, S_list, s_list, horizons, batch: int = 64, pointwise: bool = False, grid_cap: int = 0):
        """pht_ctx_forecast: for each draw (S, s), each censored observation
        c_i of this shard (a unit still in service at age c_i) and each horizon
        h the conditional failure probability q = P(T <= c_i + h | T > c_i)
        (include/pht_forecast.h), by ``loglik_unif``'s evaluator (its limits
        apply: pi = e_1, mu (c + h) up to roughly 1500).  At most 16 horizons,
        finite, >= 0 and strictly increasing; at most 2^22 censored units.

        Returns ``M`` and ``V`` [draws, H] (floats: the mean and the variance
        of that draw's Poisson-binomial number of failures within h, summed
        over the units good for that draw and horizon), ``nbad`` and ``nunits``
        [draws, H] (units that were bad there — beyond the table or below
        2^-900, never summed — and good), ``words`` (int64 [draws, H, 4] =
        [M 2^40, V 2^40, nbad, nunits]: exact integer sums, shards and ranks
        add them, ``forecast_combine``), ``qsum`` and ``cnt`` [units, H] (the
        sum of q over the draws in which the unit was good, in draw order, and
        their number), ``p_unit`` = qsum / cnt (the posterior mean failure
        probability of each unit; NaN where cnt is 0), ``unit_index`` (the
        units' indices in the order given to ``set_obs``), ``bad_draw`` and
        ``flags`` as ``loglik_unif`` gives them (a flagged draw is skipped:
        words zero, cnt untouched), and with ``pointwise`` ``q`` [draws,
        units, H] (NaN where bad; for tests and small fleets).  ``grid_cap``:
        most blocks of the kernel (0: the default); the result does not depend
        on it.  ``last_forecast_ms`` then holds the device time of the table
        kernel and of the evaluations."""
        S_all, s_all, nd = _pack_draws(S_list, s_list, self.n)
        h = np.ascontiguousarray(np.atleast_1d(horizons), np.float64).reshape(-1)
        H = len(h)
        idx = self.forecast_units()
        nc = len(idx)
        words = np.zeros((nd, max(H, 1), 4), np.int64)
        qsum, cnt = np.zeros((nc, max(H, 1))), np.zeros((nc, max(H, 1)), np.int64)
        q = np.full((nd, nc, max(H, 1)), np.nan) if pointwise else None
        flags = np.zeros(nd, np.int32)
        if self.L.pht_ctx_forecast_grid_cap(self.ctx, int(grid_cap)) != 0:
            raise _err(self.L)
        if self.L.pht_ctx_forecast(self.ctx, nd, S_all.reshape(-1), s_all.reshape(-1), H, h if H else np.zeros(1),
                                   int(batch), words.reshape(-1), qsum.ctypes.data, cnt.ctypes.data,
                                   q.ctypes.data if pointwise else None, flags) != 0:
            raise _err(self.L)
        self.last_forecast_ms = _ms_pair(self.L.pht_ctx_forecast_ms, self.ctx)
        return forecast_finalise(words, qsum, cnt, idx, flags, q)

    def condition(self, S_list, s_list, horizons=None, batch: int = 64, pointwise: bool = False, grid_cap: int = 0):
        """pht_ctx_condition: for each draw (S, s) and each censored observation
        c_i of this shard (a unit still in service at age c_i) the posterior law
        phi of the PHASE the unit is in given that it has survived to c_i, its
        mean residual life MRL = phi . (-S)^-1 1 and, for each of ``horizons``
        (none, or up to 16 as in ``forecast``), the expected number of failures
        D within h when every failed unit is replaced by a new one
        (include/pht_condition.h; ``loglik_unif``'s limits apply: pi = e_1, mu c
        up to roughly 1500, and mu h up to roughly 1450).

        Returns ``Phi`` [draws, n] (the expected number of units in each phase),
        ``L`` [draws] (the fleet's total mean residual life), ``Delta`` [draws,
        H] (the expected failures of the fleet with replacement), ``nbad`` and
        ``nunits`` [draws] (units that were bad for the draw, never summed, and
        good), ``words`` (int64 [draws, n + H + 3]: exact integer sums, shards
        and ranks add them, ``condition_combine``) with ``scales`` [draws, 1 +
        H] (the powers of two L and Delta are scaled by; they depend on the
        draw alone), ``phisum`` [units, n], ``mrlsum`` [units], ``dsum`` [units,
        H] and ``cnt`` [units] (the sums over the draws in which the unit was
        good, in draw order, and their number), ``p_phase``, ``mrl_unit``,
        ``demand_unit`` (those sums over cnt: the posterior means; NaN where cnt
        is 0), ``unit_index``, ``bad_draw`` and ``flags`` (``loglik_unif``'s
        flag words, ``CD_F_TRAP`` = 64: a state that cannot reach absorption,
        ``CD_F_HCAP`` = 128: mu h_max beyond the renewal table; a flagged draw is
        skipped), and with ``pointwise`` ``phi`` [draws, units, n], ``mrl``
        [draws, units] and ``d`` [draws, units, H] (NaN where bad; for tests and
        small fleets).  D is a mean: the variance of the replacement count
        within a draw is not computed here (``spares`` computes it).  ``last_condition_ms`` then holds the
        device time of the table kernels and of the unit kernel."""
        n = self.n
        S_all, s_all, nd = _pack_draws(S_list, s_list, n)
        h = np.ascontiguousarray(np.atleast_1d([] if horizons is None else horizons), np.float64).reshape(-1)
        H = len(h)
        idx = self.forecast_units()
        nc = len(idx)
        words, scales = np.zeros((nd, n + H + 3), np.int64), np.zeros((nd, 1 + H))
        phisum, mrlsum, dsum = np.zeros((nc, n)), np.zeros(nc), np.zeros((nc, H))
        cnt = np.zeros(nc, np.int64)
        phi = np.full((nd, nc, n), np.nan) if pointwise else None
        mrl = np.full((nd, nc), np.nan) if pointwise else None
        d = np.full((nd, nc, H), np.nan) if pointwise else None
        flags = np.zeros(nd, np.int32)
        if self.L.pht_ctx_condition_grid_cap(self.ctx, int(grid_cap)) != 0:
            raise _err(self.L)
        if self.L.pht_ctx_condition(self.ctx, nd, S_all.reshape(-1), s_all.reshape(-1), H, h if H else np.zeros(1),
                                    int(batch), words.reshape(-1), scales.reshape(-1), phisum.ctypes.data,
                                    mrlsum.ctypes.data, dsum.ctypes.data if H else None, cnt.ctypes.data,
                                    phi.ctypes.data if pointwise else None, mrl.ctypes.data if pointwise else None,
                                    d.ctypes.data if pointwise and H else None, flags) != 0:
            raise _err(self.L)
        self.last_condition_ms = _ms_pair(self.L.pht_ctx_condition_ms, self.ctx)
        return condition_finalise(words, scales, phisum, mrlsum, dsum, cnt, idx, flags, phi, mrl, d)

    def spares(self, S_list, s_list, horizons, batch: int = 64, pointwise: bool = False, grid_cap: int = 0):
        """pht_ctx_spares: for each draw (S, s), each censored observation c_i of
        this shard (a unit still in service at age c_i) and each of ``horizons``
        (1 to 16 as in ``forecast``) the mean D and the variance of the number
        of failures within h when every failed unit is replaced by a new one
        (include/pht_spares.h; ``condition``'s limits apply, and D, ``dsum``,
        ``Delta`` and ``flags`` are ``condition``'s bit for bit).  The draws'
        moment vectors are built on the device.

        Returns ``Delta`` and ``V`` [draws, H] (the mean and the variance of the
        fleet's replacement count given the draw: the units are independent
        then, so their variances add), ``nbad`` and ``nunits`` [draws],
        ``words`` (int64 [draws, 2 H + 2]: exact integer sums, shards and ranks
        add them, ``spares_combine``) with ``scales`` [draws, 2 H], ``dsum``,
        ``vsum``, ``d2sum`` [units, H] and ``cnt`` [units] (the sums of D, of
        the variance and of D^2 over the draws in which the unit was good, in
        draw order, and their number), ``demand_unit`` = dsum / cnt and
        ``demand_unit_sd`` = sqrt(vsum / cnt + d2sum / cnt - (dsum / cnt)^2)
        (the posterior predictive mean and sd of each unit's count; NaN where
        cnt is 0), ``unit_index``, ``bad_draw`` and ``flags``, and with
        ``pointwise`` ``d`` and ``var`` [draws, units, H] (NaN where bad; for
        tests and small fleets).  ``last_spares_ms`` then holds the device
        time of the vectors and table kernels and of the unit kernel."""
        S_all, s_all, nd = _pack_draws(S_list, s_list, self.n)
        h = np.ascontiguousarray(np.atleast_1d(horizons), np.float64).reshape(-1)
        H = len(h)
        idx = self.forecast_units()
        nc = len(idx)
        words, scales = np.zeros((nd, 2 * H + 2), np.int64), np.zeros((nd, 2 * H))
        dsum, vsum, d2sum = np.zeros((nc, H)), np.zeros((nc, H)), np.zeros((nc, H))
        cnt = np.zeros(nc, np.int64)
        d = np.full((nd, nc, H), np.nan) if pointwise else None
        var = np.full((nd, nc, H), np.nan) if pointwise else None
        flags = np.zeros(nd, np.int32)
        if self.L.pht_ctx_spares_grid_cap(self.ctx, int(grid_cap)) != 0:
            raise _err(self.L)
        if self.L.pht_ctx_spares(self.ctx, nd, S_all.reshape(-1), s_all.reshape(-1), H, h if H else np.zeros(1),
                                 int(batch), words.reshape(-1), scales.reshape(-1) if H else np.zeros(1),
                                 dsum.ctypes.data, vsum.ctypes.data, d2sum.ctypes.data, cnt.ctypes.data,
                                 d.ctypes.data if pointwise else None, var.ctypes.data if pointwise else None,
                                 flags) != 0:
            raise _err(self.L)
        self.last_spares_ms = _ms_pair(self.L.pht_ctx_spares_ms, self.ctx)
        return spares_finalise(words, scales, dsum, vsum, d2sum, cnt, idx, flags, d, var)

    def predict(self, S_list, s_list, nrep: int, key=(1, 2), rep0: int = 0, draw0: int = 0, edges=None,
                horizon: float = np.inf, max_jumps=None, batch: int = 64, pointwise: bool = False):
        """pht_ctx_predict: ``nrep`` replicated absorption times of PH(e_1, S)
        for each draw (S, s), simulated on the GPU (include/pht_predict.h),
        and their exact reductions.  Needs no observations on the context.

        Replicate r of draw d owns the Philox stream (key; rep0 + r;
        draw0 + d), so its value does not depend on nrep, batch or the launch.
        ``edges``: strictly increasing finite values (at most 1024) for the
        histogram; ``horizon``: paths are stopped there and recorded as
        y = horizon (``nsurv``); ``max_jumps`` (default and at most 2^20): a
        longer path is a bad replicate, as is a recorded y >= 2^20.

        Returns per draw ``mean``, ``var`` (unbiased), ``ymin``, ``ymax``,
        ``ndone``, ``nbad``, ``nsurv``, ``njump``; ``counts`` [draws, ne + 1]
        (bin = the number of edges <= y) and ``ecdf`` [draws, ne] (the share
        of recorded replicates below each edge); ``bad_draw`` / ``flags`` (a
        flagged draw is skipped: PRED_F_* and LL_F_*); the raw ``words``
        [draws, 8] int64 ``[Hy, Fy, Hq, Fq, ndone, nbad, nsurv, njump]`` and
        ``edges``; with ``pointwise`` ``y`` [draws, nrep] (NaN: bad) and
        ``jumps``.  words and counts are exact integer sums: replicate ranges
        and ranks add (``predict_combine``, or the int64 reduce ``gibbs`` is
        given, then ``predict_finalise``), ymin / ymax combine by min / max.
        At most 2^22 replicates per call: split longer runs by ``rep0``."""
        S_all, s_all, nd = _pack_draws(S_list, s_list, self.n)
        edges =np.zeros(0) if edges is None else np.ascontiguousarray(edges, np.float64).reshape(-1)
        ne, nrep = len(edges), int(nrep)
        if not 1 <= nrep <= PRED_MAX_REP:
            raise ValueError(f"nrep = {nrep} outside 1..2^22 (split a longer run by rep0)")
        words = np.zeros(PRED_WORDS * nd, np.int64)
        counts = np.zeros(nd * (ne + 1), np.int64)
        ymin, ymax = np.zeros(nd), np.zeros(nd)
        flags = np.zeros(nd, np.int32)
        y = np.full((nd, max(nrep, 0)), np.nan) if pointwise else None
        nj = np.zeros((nd, max(nrep, 0)), np.int32) if pointwise else None
        if self.L.pht_ctx_predict(self.ctx, nd, S_all.reshape(-1), s_all.reshape(-1), nrep, int(rep0), int(draw0),
                                  int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF, float(horizon),
                                  PRED_MAX_JUMPS if max_jumps is None else int(max_jumps), ne,
                                  edges if ne else np.zeros(1), int(batch), words, counts, ymin, ymax,
                                  y.ctypes.data if pointwise else None, nj.ctypes.data if pointwise else None,
                                  flags) != 0:
            raise _err(self.L)
        out = predict_finalise(words.reshape(nd, PRED_WORDS), counts.reshape(nd, ne + 1), ymin, ymax, flags, edges)
        if pointwise:
            out["y"], out["jumps"] = y, nj
        return out

    def loo_begin(self, ndraws: int) -> None:
        """pht_ctx_loo_begin: the device matrix [ndraws, observations] of a
        PSIS-LOO, every row unusable until filled (loo_fill); raises when it
        does not fit the device's free memory (thin the chain)."""
        if self.L.pht_ctx_loo_begin(self.ctx, int(ndraws)) != 0:
            raise _err(self.L)

    def loo_fill(self, row0: int, S_list=None, s_list=None, blocks=None, batch: int = 64, unif: bool = False):
        """Rows [row0, row0 + draws) of the matrix from draws (S, s) by
        uniformisation (``unif``) or from their spectral ``blocks``
        (pht_ctx_loo_fill_unif / pht_ctx_loo_fill).  Returns int64
        [draws, 4] totals ``[H, F, nbad, nobs]`` and the bool ``bad_draw``."""
        if unif:
            S_all, s_all, nd = _pack_draws(S_list, s_list, self.n)
            tot, flags = np.zeros(4 * nd, np.int64), np.zeros(nd, np.int32)
            if self.L.pht_ctx_loo_fill_unif(self.ctx, int(row0), nd, S_all.reshape(-1), s_all.reshape(-1), int(batch),
                                            tot, flags) != 0:
                raise _err(self.L)
            return tot.reshape(nd, 4), flags != 0
        blocks = np.ascontiguousarray(blocks, np.uint8)
        nb = self.L.pht_loglik_bytes(self.n)
        if blocks.ndim != 2 or blocks.shape[1] != nb or blocks.shape[0] < 1:
            raise ValueError(f"blocks must be [draws >= 1, {nb}] bytes for n = {self.n}")
        nd = blocks.shape[0]
        tot = np.zeros(4 * nd, np.int64)
        if self.L.pht_ctx_loo_fill(self.ctx, int(row0), nd, blocks.ctypes.data, int(batch), tot) != 0:
            raise _err(self.L)
        return tot.reshape(nd, 4), blocks[:, :8].copy().view(np.uint64).reshape(nd) != 0

    def loo_result(self) -> dict:
        """pht_ctx_loo over the rows filled so far: dict(elpd_i, khat,
        lppd_i, p_loo_i, flags, n_draws_used), the caller's observation order."""
        elpd, khat, lppd = np.zeros(self.count), np.zeros(self.count), np.zeros(self.count)
        flags = np.zeros(self.count, np.int32)
        used = C.c_int(0)
        if self.L.pht_ctx_loo(self.ctx, elpd, khat, lppd, flags, C.byref(used)) != 0:
            raise _err(self.L)
        return dict(elpd_i=elpd, khat=khat, lppd_i=lppd, p_loo_i=lppd - elpd, flags=flags, n_draws_used=used.value)

    def loo_end(self) -> None:
        """Free the PSIS-LOO matrix (pht_ctx_loo_end)."""
        if self.L.pht_ctx_loo_end(self.ctx) != 0:
            raise _err(self.L)

    def psis_loo(self, S_list, s_list, batch: int = 64, evaluator: str = "spectral", blocks=None) -> dict:
        """PSIS-LOO cross-validation of this shard's observations over the
        draws (S, s) (include/pht_psis.h; Vehtari, Gelman, Gabry 2017): the
        pointwise log-likelihood matrix is filled and kept on the device, then
        one wavefront per observation selects the tail of the importance
        ratios, fits the generalised Pareto and smooths.

        Returns per observation ``elpd_i``, ``khat`` (the Pareto shape; +inf
        where nothing was smoothed), ``lppd_i``, ``p_loo_i = lppd_i - elpd_i``
        and ``flags`` (1: an l of a usable draw is NaN, outputs NaN; 2: fewer
        than 25 usable draws; 4: constant tail; 8: no finite fit); per draw
        ``bad_draw``, ``evaluator`` and ``total`` (the log-likelihood trace,
        as Sweeper.loglik gives it); ``n_draws_used``.  ``evaluator`` and
        ``blocks`` as in Sweeper.loglik; flagged draws are left out.  At most
        16384 draws; the matrix (draws x observations x 8 bytes) must fit the
        device: thin the chain otherwise.  The WAIC state is not touched.
        Observations are independent: shards and ranks each run their own,
        and the sums over elpd_i add."""
        if evaluator not in EVALUATORS:
            raise ValueError(f"evaluator must be one of {EVALUATORS}, got {evaluator!r}")
        S_list, s_list = list(S_list), list(s_list)
        nd = len(S_list)
        if evaluator != "unif" and blocks is None:
            blocks = np.stack([loglik_block(S, s) for S, s in zip(S_list, s_list)])
        if evaluator == "unif":
            runs = [(0, nd, True)]
        elif evaluator == "spectral":
            runs = [(0, nd, False)]
        else:
            runs = self._auto_runs(blocks, batch)
        tot, bad = np.zeros((nd, 4), np.int64), np.zeros(nd, bool)
        which = np.full(nd, "spectral", dtype="<U8")
        self.loo_begin(nd)
        try:
            for lo, hi, unif in runs:
                if unif:
                    tot[lo:hi], bad[lo:hi] = self.loo_fill(lo, S_list[lo:hi], s_list[lo:hi], batch=batch, unif=True)
                    which[lo:hi] = "unif"
                else:
                    tot[lo:hi], bad[lo:hi] = self.loo_fill(lo, blocks=blocks[lo:hi], batch=batch)
            out = self.loo_result()
        finally:
            self.loo_end()
        out.update(bad_draw=bad, evaluator=which, total=loglik_total(tot[:, 0], tot[:, 1], tot[:, 2], bad))
        return out

    def waic_reset(self) -> None:
        """Forget the per-observation WAIC state (pht_ctx_loglik_reset)."""
        if self.L.pht_ctx_loglik_reset(self.ctx) != 0:
            raise _err(self.L)

    def waic_state(self):
        """The per-observation WAIC accumulators (pht_waic_t), in the caller's
        observation order: dict(ref, S1, S2, m, r, cnt)."""
        d = {k: np.zeros(self.count, np.float64) for k in ("ref", "S1", "S2", "m", "r")}
        cnt = np.zeros(self.count, np.int32)
        if self.L.pht_ctx_loglik_state(self.ctx, d["ref"], d["S1"], d["S2"], d["m"], d["r"], cnt) != 0:
            raise _err(self.L)
        d["cnt"] = cnt
        return d

    def close(self):
        if self.ctx:
            self.L.pht_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def _chains_start(start, K: int, m: int) -> np.ndarray:
    """The start block pht_gibbs_run_chains reads: [-1] (draw from the prior),
    or K*m values, chain c at [c*m, (c+1)*m).  A single m-vector (what
    Sweeper.gibbs and the R API take) is broadcast to every chain; any other
    length is refused here, because the C side reads start + c*m unchecked."""
    if start is None:
        return np.array([-1.0])
    st = np.ascontiguousarray(start, np.float64).reshape(-1)
    if st.size >= 1 and st[0] < 0:
        return np.array([-1.0])
    if st.size == m:
        return np.ascontiguousarray(np.tile(st, K))
    if st.size == K * m:
        return st
    raise ValueError(f"gibbs_chains: start has {st.size} values; need {m} (one start for every chain) "
                     f"or {K}*{m} (one per chain), or a negative first value")


def gibbs_chains(seeds, y, censored, n, method, nu, zeta, T, C_, mhit: int = 1, it: int = 100, start=None,
                 device: int = 0, obs0: int = 0):
    """Independent Gibbs chains at once (pht_gibbs_run_chains):
    chain c is the single chain of ``Sweeper.gibbs`` after ``set_seed(seeds[c])``.
    Returns (draws [chains, it, m], max kernel ms)."""
    L = load()
    seeds = np.ascontiguousarray(seeds, np.uint32)
    K, m = len(seeds), len(nu)
    sws = []
    try:
        for _ in range(K):
            sw = Sweeper(n, method, mhit, device=device)
            sw.set_obs(y, censored, obs0=obs0)
            sws.append(sw)
        ctxs = (C.c_void_p * K)(*[sw.ctx for sw in sws])
        res = np.zeros(K * it * m, np.float64)
        st = _chains_start(start, K, m)
        Tf = np.ascontiguousarray(np.asarray(T).reshape(-1, order="F"), np.int32)
        Cf = np.ascontiguousarray(np.asarray(C_, np.float64).reshape(-1, order="F"))
        kms = C.c_double(0.0)
        zexp = zexp_for(y)
        if L.pht_gibbs_run_chains(ctxs, K, seeds, it, method, m, np.ascontiguousarray(nu, np.float64),
                                  np.ascontiguousarray(zeta, np.float64), Tf, Cf, zexp, st, res,
                                  C.byref(kms)) != 0:
            raise _err(L)
        return res.reshape(K, m, it).transpose(0, 2, 1).copy(), kms.value
    finally:
        for sw in sws:
            sw.close()


def LJMA_Gibbs(it, mhit, method, n, m, nu, zeta, T, C_, y, l, censored, start, silent, res):
    """The .C routine (src/PHT_MCMC_Aslett.c:104) with R's .C semantics:
    every argument is a fresh vector; returns the dict of (modified) vectors."""
    L = load()
    a = dict(it=np.array([it], np.int32), mhit=np.array([mhit], np.int32), method=np.array([method], np.int32),
             n=np.array([n], np.int32), m=np.array([m], np.int32), nu=np.array(nu, np.float64),
             zeta=np.array(zeta, np.float64), T=np.array(T, np.int32).reshape(-1, order="F"),
             C=np.array(C_, np.float64).reshape(-1, order="F"), y=np.array(y, np.float64),
             l=np.array([l], np.int32), censored=np.array(censored, np.int32), start=np.array(start, np.float64),
             silent=np.array([silent], np.int32), res=np.array(res, np.float64))
    a = {k: np.ascontiguousarray(v) for k, v in a.items()}
    L.LJMA_Gibbs(*a.values())
    msg = L.pht_last_error().decode()
    if msg:
        raise PhaseTypeError(msg)
    return a


def _r_sort(names, collation: str = "C"):
    """R's sort() of character names.  "C": byte order; "en_US": case-folded
    first (how a typical UTF-8 locale collates S12 / s1)."""
    if collation == "C":
        return sorted(names)
    return sorted(names, key=lambda s: (s.lower(), s.swapcase()))


def phtMCMC2(x, TT, beta, nu, zeta, n, censored=None, C_=None, method="ECS", mhit=1, resume=None,
             silent=False, collation="C"):
    """R/phtMCMC2.R:1-86: structured generator TT (strings, "0" = fixed zero)."""
    TT = np.asarray(TT, dtype=object).astype(str)
    nu = {k: float(nu[k]) for k in _r_sort(list(nu), collation)}
    zeta = {k: float(zeta[k]) for k in _r_sort(list(zeta), collation)}
    if int(n) < 1:
        raise ValueError(f"{n} is an invalid number of MCMC iterations.")
    if int(mhit) < 0:
        raise ValueError(f"{mhit} is an invalid number of Metropolis-Hastings iterations.")
    dimT = TT.shape[0]
    if TT.shape[0] != TT.shape[1]:
        raise ValueError("matrix of variables must be square")
    if set(np.diag(TT)) != {"0"}:
        raise ValueError("diagonal of matrix of variables must be zeros")
    if set(TT[dimT - 1, :]) != {"0"}:
        raise ValueError("last row of matrix of variables must represent absorbing state (and so be all zeros)")
    if len(beta) != dimT - 1:
        raise ValueError(f"beta should be a vector of length {dimT - 1} for the generator specified.")
    if any(b < 0 for b in beta):
        raise ValueError("beta is not a valid parameter of a Dirichlet distribution.")
    if C_ is None:
        C_ = np.ones((dimT, dimT))
    C_ = np.asarray(C_, np.float64)
    if C_.shape != (dimT, dimT):
        raise ValueError("dimension of C must match dimension of TT")
    var_names = [v for v in _r_sort(set(TT.reshape(-1)), collation) if v != "0"]
    if list(nu) != var_names:
        raise ValueError("variables specified in matrix don't match those in prior nu")
    if list(zeta) != var_names:
        raise ValueError("variables specified in matrix don't match those in prior zeta")
    start = [-1.0]
    it = int(n)
    if resume is not None:
        resume = np.asarray(resume, np.float64)
        if resume.shape[1] != len(var_names):
            raise ValueError("the variables in resume do not match the variables in generator")
        start = list(resume[-1])
        it = it + 1
    TN = np.zeros((dimT, dimT), np.int32)
    for i in range(dimT):
        for j in range(dimT):
            TN[i, j] = (["0"] + var_names).index(TT[i, j])
    meths = [method] if isinstance(method, str) else list(method)
    bad = set(meths) - set(METHODS)
    if bad:
        raise ValueError(f"Error: unknown sampling methods ({', '.join(sorted(bad))})")
    method_num = sum(METHODS[k] for k in dict.fromkeys(meths))
    x = np.asarray(x, np.float64)
    cen = np.zeros(len(x), np.int32) if censored is None else np.asarray(censored).astype(np.int32)
    out = LJMA_Gibbs(it, mhit, method_num, dimT - 1, len(var_names), list(nu.values()), list(zeta.values()), TN,
                     C_, x, len(x), cen, start, int(silent), np.zeros(it * len(var_names)))
    samples = out["res"].reshape(len(var_names), it).T
    if resume is not None:
        samples = np.vstack([resume[:-1], samples])
    return dict(samples=samples, data=x, vars=var_names, TT=TT, beta=beta, nu=nu, zeta=zeta, iterations=it,
                censored=cen, method=method, MHit=mhit)


def phtMCMC(x, states, beta, nu, zeta, n, mhit=1, resume=None, silent=False, collation="C"):
    """R/phtMCMC.R:1-97: dense generator, always MHRS."""
    if len(nu) != states * states:
        raise ValueError("nu must specify one prior Gamma shape parameter per element of the Phase-type generator")
    if len(zeta) != states:
        raise ValueError("zeta must specify one prior Gamma reciprocal scale parameter per non-absorbing row")
    TT = np.empty((states + 1, states + 1), dtype=object)
    for i in range(states):
        for j in range(states):
            TT[i, j] = f"S{i + 1}{j + 1}"
        TT[i, states] = f"s{i + 1}"
    TT[states, :] = "0"
    for i in range(states + 1):
        TT[i, i] = "0"
    names = [v for v in TT.T.T.reshape(-1) if v != "0"]  # c(t(TT)) without "0": row-major
    nu_d = dict(zip(names, [float(v) for v in nu]))
    # zeta <- as.list(rep(zeta, each=states+1)); names(zeta) <- names (R/phtMCMC.R:29-30)
    zrep = np.repeat(np.asarray(zeta, np.float64), states + 1)
    zeta_d = dict(zip(names, zrep[:len(names)]))
    return phtMCMC2(x, TT, beta, nu_d, zeta_d, n, censored=None, C_=np.ones((states + 1, states + 1)),
                    method="MHRS", mhit=mhit, resume=resume, silent=silent, collation=collation)


# ------------------------------------------------- log-likelihood of the draws
# No reference counterpart: the reference returns the draws only.  The
# arithmetic is specified in include/pht_loglik.h and runs in
# phasetype_amd/csrc/pht_loglik.hip: the spectral evaluator, the default (a
# draw with a complex spectrum, or with a defective or nearly defective one
# whose coefficients cancel past the guard, is flagged, reported as NaN and
# never evaluated; an observation whose sum cancels past it is bad for that
# draw).  The second evaluator, by uniformisation, serves those draws:
# include/pht_loglik_unif.h, phasetype_amd/csrc/pht_loglik_unif.hip.
EVALUATORS = ("spectral", "unif", "auto")
LL_F_INFO, LL_F_COMPLEX, LL_F_NONFINITE, LL_F_MU, LL_F_ILLCOND = 1, 2, 4, 8, 16  # flag words (pht_loglik.h, pht_loglik_unif.h)


def evaluator_runs(flags, nbad=None) -> list:
    """evaluator="auto": the draw sequence split into maximal runs of one
    evaluator, in order, as [(lo, hi, unif)] over draws [lo, hi).  ``flags``:
    the draws' spectral block flag words.  A draw goes to uniformisation where
    its spectrum is complex, defective or so nearly defective that its
    coefficients cancel (LL_F_COMPLEX, LL_F_INFO, LL_F_ILLCOND) and its
    generator finite, and where its block is usable but its spectral
    evaluation left bad observations (``nbad``: per draw, from a totals-only
    spectral pass; None: not looked at); otherwise to the spectral evaluator
    (flag 0: evaluated; LL_F_NONFINITE: NaN from either)."""
    flags = np.asarray(flags).astype(np.uint64).reshape(-1)
    unif = (((flags & np.uint64(LL_F_INFO | LL_F_COMPLEX | LL_F_ILLCOND)) != 0)
            & ((flags & np.uint64(LL_F_NONFINITE)) == 0))
    if nbad is not None:
        unif = unif | ((flags == 0) & (np.asarray(nbad).reshape(-1) > 0))
    runs, lo = [], 0
    for k in range(1, len(unif) + 1):
        if k == len(unif) or unif[k] != unif[lo]:
            runs.append((lo, k, bool(unif[lo])))
            lo = k
    return runs


def loglik_block(S, s) -> np.ndarray:
    """One draw's block for ``Sweeper.loglik_blocks`` (pht_loglik_build; host
    only): uint8[pht_loglik_bytes(n)].  An unusable draw (complex spectrum,
    failed LAPACK call, non-finite entry, or coefficients that cancel past
    the guard, LL_F_ILLCOND: every exactly defective spectrum and the nearly
    defective ones) has a non-zero first word."""
    L = load()
    S = np.asarray(S, np.float64)
    n = S.shape[0]
    nb = L.pht_loglik_bytes(n)
    if nb < 0 or S.shape != (n, n):
        raise ValueError(f"S must be square with 1 <= n <= 32, got {S.shape}")
    out = np.zeros(nb, np.uint8)
    Sf = np.ascontiguousarray(S.reshape(-1, order="F"))
    if L.pht_loglik_build(n, Sf, np.ascontiguousarray(s, np.float64), out.ctypes.data, nb) < 0:
        raise _err(L)
    return out


def loglik_total(H, F, nbad, bad_draw) -> np.ndarray:
    """The log-likelihood per draw from its (summed) fixed-point words:
    H + F 2^-32; -inf where an observation was bad; NaN for an unusable draw."""
    H, F = np.asarray(H, np.int64), np.asarray(F, np.int64)
    tot = H.astype(np.float64) + F.astype(np.float64) * 2.0 ** -32
    tot = np.where(np.asarray(nbad) > 0, -np.inf, tot)
    return np.where(np.asarray(bad_draw, bool), np.nan, tot)


def _tt_numbers(TT_or_T, collation: str = "C"):
    """(T as int32 [n+1, n+1], variable names or None): a matrix of names is
    numbered as phtMCMC2 does (sorted names without "0" -> 1..m, which is the
    column order of its samples); a matrix of integers is taken as T."""
    A = np.asarray(TT_or_T)
    if A.ndim != 2 or A.shape[0] != A.shape[1] or A.shape[0] < 2:
        raise ValueError("matrix of variables must be square")
    if A.dtype.kind in "iu":
        return np.ascontiguousarray(A, np.int32), None
    TT = np.asarray(TT_or_T, dtype=object).astype(str)
    var_names = [v for v in _r_sort(set(TT.reshape(-1)), collation) if v != "0"]
    TN = np.zeros(TT.shape, np.int32)
    for i in range(TT.shape[0]):
        for j in range(TT.shape[1]):
            TN[i, j] = (["0"] + var_names).index(TT[i, j])
    return TN, var_names


def theta_to_S(theta, T, C_=None):
    """One row of a chain -> (S [n, n], s [n]) (pht_theta_to_S: the T / C maps
    of the Gibbs loop; T numbers as ``_tt_numbers`` gives them)."""
    L = load()
    T = np.asarray(T, np.int32)
    n1 = T.shape[0]
    n = n1 - 1
    C_ = np.ones((n1, n1)) if C_ is None else np.asarray(C_, np.float64)
    theta = np.ascontiguousarray(theta, np.float64)
    S, s = np.zeros(n * n), np.zeros(n)
    Tf = np.ascontiguousarray(T.reshape(-1, order="F"), np.int32)
    Cf = np.ascontiguousarray(C_.reshape(-1, order="F"), np.float64)
    if L.pht_theta_to_S(n, len(theta), Tf, Cf, theta, S, s) != 0:
        raise _err(L)
    return S.reshape(n, n, order="F"), s


def _chain_draws(res, TT_or_T, C_, n, collation="C"):
    """(S_list, s_list, n) for the rows of a chain: ``res`` is the dict
    phtMCMC2 / phtMCMC return or the it x m array of Sweeper.gibbs."""
    if isinstance(res, dict):
        samples = np.asarray(res["samples"], np.float64)
        if TT_or_T is None:
            TT_or_T = res["TT"]
    else:
        samples = np.asarray(res, np.float64)
    samples = np.atleast_2d(samples)
    T, names = _tt_numbers(TT_or_T, collation)
    if n is not None and int(n) != T.shape[0] - 1:
        raise ValueError(f"n = {n} does not match the {T.shape[0]} x {T.shape[0]} generator")
    if isinstance(res, dict) and names is not None and list(res.get("vars", names)) != names:
        raise ValueError("the variables of the chain do not match the variables in the generator")
    if samples.shape[1] != int(T.max()):
        raise ValueError(f"the chain has {samples.shape[1]} columns, the generator {int(T.max())} variables")
    draws = [theta_to_S(row, T, C_) for row in samples]
    return [d[0] for d in draws], [d[1] for d in draws], T.shape[0] - 1


def _chain_blocks(res, TT_or_T, C_, n, collation="C"):
    """(blocks uint8 [draws, bytes], n) for the rows of a chain (_chain_draws)."""
    S_list, s_list, n = _chain_draws(res, TT_or_T, C_, n, collation)
    return np.stack([loglik_block(S, s) for S, s in zip(S_list, s_list)]), n


def _obs_sweeper(x, censored, n, device):
    sw = Sweeper(n, METHODS["ECS"], 1, device=device)
    sw.set_obs(np.asarray(x, np.float64), censored)
    return sw


def log_lik(res, x, TT_or_T=None, censored=None, C_=None, n=None, device: int = 0, batch: int = 64,
            collation: str = "C", evaluator: str = "spectral") -> np.ndarray:
    """The observed-data log-likelihood trace of a chain: one value per row of
    ``res`` (the dict phtMCMC2 / phtMCMC return, or the array of
    Sweeper.gibbs), over data ``x`` / ``censored``.  ``TT_or_T``: the matrix of
    variable names given to phtMCMC2 (numbered as it numbers them; default the
    chain's own) or the integer matrix T of Sweeper.gibbs.  NaN for a flagged
    draw (a complex spectrum; a defective or nearly defective one, as every
    draw of a structure with one rate on several transitions has:
    LL_F_ILLCOND), -inf where an observation has no density or its sum cancels
    past the guard.  ``evaluator`` (Sweeper.loglik): "unif" or "auto" evaluate
    those draws too, by uniformisation."""
    S_list, s_list, n = _chain_draws(res, TT_or_T, C_, n, collation)
    sw = _obs_sweeper(x, censored, n, device)
    try:
        return sw.loglik(S_list, s_list, batch=batch, evaluator=evaluator)["total"]
    finally:
        sw.close()


def waic_from_state(st) -> dict:
    """WAIC from the per-observation accumulators (Sweeper.waic_state):
    lppd_i = m + log r - log cnt, p_waic_i = (S2 - S1^2 / cnt) / (cnt - 1)."""
    cnt = np.asarray(st["cnt"], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        lppd_i = st["m"] + np.log(st["r"]) - np.log(cnt)
        p_i = (st["S2"] - st["S1"] ** 2 / cnt) / (cnt - 1.0)
    lppd, p = float(np.sum(lppd_i)), float(np.sum(p_i))
    return dict(elpd_waic=lppd - p, p_waic=p, lppd=lppd, waic=-2.0 * (lppd - p), pointwise=(lppd_i, p_i),
                n_draws_used=int(np.max(st["cnt"])) if len(cnt) else 0)


def waic(res, x, TT_or_T=None, censored=None, C_=None, n=None, burn: int = 0, device: int = 0, batch: int = 64,
         collation: str = "C", evaluator: str = "spectral") -> dict:
    """WAIC of a chain (rows from ``burn`` on) over data ``x`` / ``censored``:
    dict(elpd_waic, p_waic, lppd, waic, pointwise=(lppd_i, p_waic_i),
    n_draws_used).  Flagged draws (a complex spectrum, or coefficients that
    cancel: Sweeper.loglik_blocks) are left out by the default ``evaluator``; "auto" (Sweeper.loglik) evaluates them by
    uniformisation, in the chain's order, and n_draws_used then counts every
    finite draw."""
    S_list, s_list, n = _chain_draws(res, TT_or_T, C_, n, collation)
    sw = _obs_sweeper(x, censored, n, device)
    try:
        sw.waic_reset()
        r = sw.loglik(S_list[int(burn):], s_list[int(burn):], batch=batch, accumulate=True, evaluator=evaluator)
        out = waic_from_state(sw.waic_state())
        out["n_draws_used"] = int(np.sum(~r["bad_draw"]))
        return out
    finally:
        sw.close()


def ph_curves(res, TT_or_T, grid, C_=None, n=None, device: int = 0, batch: int = 64, collation: str = "C",
              evaluator: str = "spectral") -> dict:
    """Per-draw curves on ``grid``: dict(logdens, logsurv, hazard), each
    [draws, len(grid)] (the grid as exact, then as censored observations, in
    pointwise mode).  Bands: ``np.quantile(out["hazard"], [.025, .975], axis=0)``.
    ``evaluator``: as in Sweeper.loglik."""
    S_list, s_list, n = _chain_draws(res, TT_or_T, C_, n, collation)
    blocks = None if evaluator == "unif" else np.stack([loglik_block(S, s) for S, s in zip(S_list, s_list)])
    grid = np.ascontiguousarray(grid, np.float64)
    sw = Sweeper(n, METHODS["ECS"], 1, device=device)
    kw = dict(batch=batch, pointwise=True, evaluator=evaluator, blocks=blocks)
    try:
        sw.set_obs(grid, np.zeros(len(grid), np.int32))
        ld = sw.loglik(S_list, s_list, **kw)["pointwise"]
        sw.set_obs(grid, np.ones(len(grid), np.int32))
        ls = sw.loglik(S_list, s_list, **kw)["pointwise"]
    finally:
        sw.close()
    return dict(logdens=ld, logsurv=ls, hazard=np.exp(ld - ls))


# ------------------------------------------------- the d / p / q / r family
# include/pht_quantile.h, phasetype_amd/csrc/pht_quantile.hip (no reference
# counterpart); rph is further down with the posterior-predictive replicates
Q_F_P, Q_F_T0, Q_F_BEYOND, Q_F_EVAL, Q_F_CAP, Q_F_DRAW = 1, 2, 4, 8, 16, 32


def quantile_host(S, s, probs, given: float = 0.0, tmax=None) -> dict:
    """pht_quantile_host (host only, no GPU): ``Sweeper.quantile``'s dict for
    one draw, each array [P]; bit for bit what the device computes."""
    L = load()
    S = np.asarray(S, np.float64)
    n = S.shape[0]
    probs = np.ascontiguousarray(np.atleast_1d(probs), np.float64).reshape(-1)
    P_ = len(probs)
    t, lo, hi = np.zeros(P_), np.zeros(P_), np.zeros(P_)
    nev, flags = np.zeros(P_, np.int32), np.zeros(P_, np.uint32)
    f = L.pht_quantile_host(n, np.ascontiguousarray(S.reshape(-1, order="F")),
                            np.ascontiguousarray(s, np.float64).reshape(-1), P_, probs, float(given),
                            np.inf if tmax is None else float(tmax), t, lo, hi, nev, flags)
    if f < 0:
        raise _err(L)
    return dict(t=t, lo=lo, hi=hi, nev=nev, flags=flags, bad_draw=f != 0, draw_flags=f)


def qph(S, s, p, given: float = 0.0, device: int = 0):
    """The quantile function of PH(e_1, S): the t with P(T <= t) = p, or with
    ``given`` = t0 > 0 the residual life t - t0 with P(T <= t | T > t0) = p
    (Sweeper.quantile on one draw; the shape of ``p``).  inf for p = 1 and for
    a root beyond 1400 / the largest rate; NaN for a p outside [0, 1]."""
    S = np.asarray(S, np.float64)
    sw = Sweeper(S.shape[0], METHODS["ECS"], 1, device=device)
    try:
        r = sw.quantile([S], [s], np.asarray(p, np.float64).reshape(-1), given=given)
        if r["bad_draw"][0]:
            raise ValueError(f"not a usable generator (flag {r['draw_flags'][0]})")
        t = r["t"][0].reshape(np.shape(p))
        return float(t) if np.ndim(p) == 0 else t
    finally:
        sw.close()


def _pointwise_unif(S, s, t, cens, device):
    S = np.asarray(S, np.float64)
    t = np.asarray(t, np.float64)
    sw = Sweeper(S.shape[0], METHODS["ECS"], 1, device=device)
    try:
        sw.set_obs(t.reshape(-1), np.full(t.size, cens, np.int32))
        l = sw.loglik_unif([S], [s], pointwise=True)["pointwise"][0].reshape(t.shape)
        return float(l) if t.ndim == 0 else l
    finally:
        sw.close()


def dph(S, s, t, device: int = 0):
    """The density of PH(e_1, S) at ``t``: exp of the uniformisation
    evaluator's pointwise log-likelihood of exact observations."""
    return np.exp(_pointwise_unif(S, s, t, 0, device))


def pph(S, s, t, device: int = 0):
    """The distribution function of PH(e_1, S) at ``t``: 1 - exp(log survival),
    the evaluator's pointwise log-likelihood of censored observations."""
    return -np.expm1(_pointwise_unif(S, s, t, 1, device))


def ph_quantiles(res, TT_or_T, probs, given: float = 0.0, C_=None, n=None, burn: int = 0, thin: int = 1, tmax=None,
                 device: int = 0, batch: int = 64, collation: str = "C", band=(.025, .5, .975)) -> dict:
    """Posterior quantiles of a chain (``res`` and ``TT_or_T`` as in
    ``log_lik``; rows ``burn::thin``): dict(q [draws, P], the quantile (or,
    with ``given`` > 0, the residual-life quantile) of every draw at every
    probability; band [len(band), P], the posterior ``band`` quantiles of each
    column over its finite entries (NaN where none is); n_finite [P];
    n_beyond [P], draws whose root lies beyond the horizon (inf in q);
    n_flagged [P], draws that gave NaN (a flagged draw or root); flags
    [draws, P], bad_draw [draws], lo, hi, nev).  Nothing is dropped silently:
    n_finite + n_beyond + n_flagged = draws, but for p = 1 (inf, no flag)."""
    S_list, s_list, n = _chain_draws(res, TT_or_T, C_, n, collation)
    S_list, s_list = S_list[int(burn)::int(thin)], s_list[int(burn)::int(thin)]
    if not S_list:
        raise ValueError("no rows left after burn / thin")
    sw = Sweeper(n, METHODS["ECS"], 1, device=device)
    try:
        r = sw.quantile(S_list, s_list, probs, given=given, tmax=tmax, batch=batch)
    finally:
        sw.close()
    q = r["t"]
    fin = np.isfinite(q)
    bands = np.full((len(band), q.shape[1]), np.nan)
    for j in range(q.shape[1]):
        if fin[:, j].any():
            bands[:, j] = np.quantile(q[fin[:, j], j], band)
    return dict(q=q, band=bands, n_finite=fin.sum(0), n_beyond=((r["flags"] & Q_F_BEYOND) != 0).sum(0),
                n_flagged=np.isnan(q).sum(0), flags=r["flags"], bad_draw=r["bad_draw"], lo=r["lo"], hi=r["hi"],
                nev=r["nev"], probs=np.atleast_1d(np.asarray(probs, np.float64)))


# ------------------------------------------------------------ fleet forecasts
# include/pht_forecast.h, phasetype_amd/csrc/pht_forecast.hip (no reference
# counterpart): which of the units still in service fail within h, and how many
FORECAST_MAX_H, FORECAST_MAX_UNITS, FORECAST_SCALE = 16, 1 << 22, 2.0 ** 40


def forecast_finalise(words, qsum, cnt, unit_index, flags, q=None) -> dict:
    """``Sweeper.forecast``'s dict from the raw outputs (words int64 [draws, H,
    4], qsum and cnt [units, H], the units' indices, the draws' flag words)."""
    words = np.asarray(words, np.int64)
    qsum, cnt = np.asarray(qsum, np.float64), np.asarray(cnt, np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        p_unit = np.where(cnt > 0, qsum / np.maximum(cnt, 1), np.nan)
    flags = np.asarray(flags, np.int32)
    out = dict(M=words[:, :, 0] / FORECAST_SCALE, V=words[:, :, 1] / FORECAST_SCALE, nbad=words[:, :, 2].copy(),
               nunits=words[:, :, 3].copy(), words=words, p_unit=p_unit, qsum=qsum, cnt=cnt,
               unit_index=np.asarray(unit_index, np.int64), bad_draw=flags != 0, flags=flags)
    if q is not None:
        out["q"] = q
    return out


def forecast_host(S, s, ages, horizons, ymax_c: float = 0.0, state=None) -> dict:
    """pht_forecast_host (host only, no GPU): ``Sweeper.forecast``'s dict for
    one draw over units of the given ``ages``, with ``q`` [1, units, H]; bit for
    bit what the device computes.  ``ymax_c``: the largest censored observation
    the table is sized for (0: the largest age).  ``state``: the dict of the
    chain's earlier draws, whose ``qsum`` and ``cnt`` this draw continues (its
    words are not kept)."""
    L = load()
    S = np.asarray(S, np.float64)
    n = S.shape[0]
    ages = np.ascontiguousarray(np.atleast_1d(ages), np.float64).reshape(-1)
    h = np.ascontiguousarray(np.atleast_1d(horizons), np.float64).reshape(-1)
    nc, H = len(ages), len(h)
    words = np.zeros((1, max(H, 1), 4), np.int64)
    if state is None:
        qsum, cnt = np.zeros((nc, max(H, 1))), np.zeros((nc, max(H, 1)), np.int64)
    else:
        qsum, cnt = np.array(state["qsum"], np.float64), np.array(state["cnt"], np.int64)
        if qsum.shape != (nc, H) or cnt.shape != (nc, H):
            raise ValueError("state does not have this call's units and horizons")
    q = np.full((1, nc, max(H, 1)), np.nan)
    f = L.pht_forecast_host(n, np.ascontiguousarray(S.reshape(-1, order="F")),
                            np.ascontiguousarray(s, np.float64).reshape(-1), nc, ages if nc else np.zeros(1), H,
                            h if H else np.zeros(1), float(ymax_c), words.reshape(-1), qsum.ctypes.data,
                            cnt.ctypes.data, q.ctypes.data)
    if f < 0:
        raise _err(L)
    return forecast_finalise(words, qsum, cnt, np.arange(nc), np.array([f], np.int32), q)


def forecast_combine(a: dict, b: dict) -> dict:
    """The forecast of two shards' units from the forecasts of each
    (``Sweeper.forecast`` of the same draws and horizons on each shard): the
    words add exactly, the per-unit blocks concatenate (``b``'s units after
    ``a``'s; ``unit_index`` stays each shard's own numbering)."""
    if a["words"].shape != b["words"].shape or not np.array_equal(a["flags"], b["flags"]):
        raise ValueError("the two forecasts are not of the same draws and horizons")
    q = np.concatenate([a["q"], b["q"]], axis=1) if ("q" in a and "q" in b) else None
    return forecast_finalise(a["words"] + b["words"], np.concatenate([a["qsum"], b["qsum"]]),
                             np.concatenate([a["cnt"], b["cnt"]]),
                             np.concatenate([a["unit_index"], b["unit_index"]]), a["flags"], q)


def forecast_moments(M, V, use=None) -> dict:
    """The predictive moments of the number of failures per horizon from the
    draws' Poisson-binomial moments ``M``, ``V`` [draws, H] (``use``: which
    [draw, horizon] cells count; default all): ``mean`` = mean_d M_d, ``within``
    = mean_d V_d, ``between`` = the variance of M_d over the draws (the
    mixture's own: divided by the number of draws), ``sd`` = sqrt(within +
    between) by the law of total variance, ``n_used`` draws per horizon."""
    M, V = np.atleast_2d(np.asarray(M, np.float64)), np.atleast_2d(np.asarray(V, np.float64))
    use = np.ones(M.shape, bool) if use is None else np.asarray(use, bool)
    k = use.sum(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(use, M, 0.0).sum(0) / k
        within = np.where(use, V, 0.0).sum(0) / k
        between = np.where(use, (M - mean) ** 2, 0.0).sum(0) / k
    return dict(mean=mean, within=within, between=between, sd=np.sqrt(within + between), n_used=k)


def forecast_count_quantiles(M, V, p, use=None) -> np.ndarray:
    """Quantiles [len(p), H] of the predictive number of failures per horizon,
    APPROXIMATED by the equal-weight mixture over the draws of normals matched
    to each draw's (M_d, V_d): the x with mean_d Phi((x - M_d) / sqrt(V_d)) = p,
    by bisection (a draw with V_d = 0 is a step at M_d).  Continuous, not
    rounded to counts; a Poisson-binomial law of few units or of tiny
    probabilities is skewed and discrete, which a normal is not (DESIGN.md 5i
    records the difference against the exact law)."""
    from scipy.special import ndtr

    M, V = np.atleast_2d(np.asarray(M, np.float64)), np.atleast_2d(np.asarray(V, np.float64))
    use = np.ones(M.shape, bool) if use is None else np.asarray(use, bool)
    p = np.atleast_1d(np.asarray(p, np.float64))
    out = np.full((len(p), M.shape[1]), np.nan)
    for j in range(M.shape[1]):
        m, sd = M[use[:, j], j], np.sqrt(np.maximum(V[use[:, j], j], 0.0))
        if not len(m):
            continue

        def cdf(x):
            with np.errstate(divide="ignore", invalid="ignore"):
                z = np.where(sd > 0, (x - m) / np.where(sd > 0, sd, 1.0), np.where(x >= m, np.inf, -np.inf))
            return float(np.mean(ndtr(z)))

        lo0, hi0 = float(np.min(m - 40.0 * sd)) - 1.0, float(np.max(m + 40.0 * sd)) + 1.0
        for i, pv in enumerate(p):
            if not 0.0 < pv < 1.0:
                continue
            lo, hi = lo0, hi0
            for _ in range(200):
                mid = 0.5 * (lo + hi)
                if cdf(mid) < pv:
                    lo = mid
                else:
                    hi = mid
                if hi - lo <= 1e-12 * max(1.0, abs(hi)):
                    break
            out[i, j] = hi
    return out


def fleet_forecast(res, x, TT_or_T, horizons, censored, C_=None, n=None, burn: int = 0, thin: int = 1,
                   device: int = 0, batch: int = 64, collation: str = "C") -> dict:
    """The forecast of a fleet from a chain (``res`` and ``TT_or_T`` as in
    ``log_lik``; rows ``burn::thin``): of the units of ``x`` still in service
    (``censored`` != 0, at age x_i), how many fail within each of ``horizons``,
    and which.  ``Sweeper.forecast``'s dict plus, per horizon, ``mean`` (the
    expected number of failures), ``sd`` (the predictive standard deviation by
    the law of total variance) with its two parts ``within`` = mean_d V_d (the
    units' own randomness) and ``between`` = var_d M_d (the posterior's),
    ``n_used`` (the draws that count for that horizon: not flagged and with no
    bad unit there; ``mean`` is NaN where none does), ``count_quantiles(p)``
    (``forecast_count_quantiles``: an approximation) and ``ranking`` [H, units]
    (the units, as rows of ``p_unit``, by decreasing ``p_unit``, NaN last)."""
    S_list, s_list, n = _chain_draws(res, TT_or_T, C_, n, collation)
    S_list, s_list = S_list[int(burn)::int(thin)], s_list[int(burn)::int(thin)]
    if not S_list:
        raise ValueError("no rows left after burn / thin")
    sw = _obs_sweeper(x, censored, n, device)
    try:
        r = sw.forecast(S_list, s_list, horizons, batch=batch)
    finally:
        sw.close()
    use = (~r["bad_draw"])[:, None] & (r["nbad"] == 0)
    r.update(forecast_moments(r["M"], r["V"], use))
    M, V = r["M"], r["V"]
    r["count_quantiles"] = lambda p: forecast_count_quantiles(M, V, p, use)
    key = np.where(np.isnan(r["p_unit"]), -np.inf, r["p_unit"])
    r["ranking"] = np.argsort(-key, axis=0, kind="stable").T
    r["horizons"] = np.atleast_1d(np.asarray(horizons, np.float64))
    return r


# ------------------------------------------------------------ fleet condition
# include/pht_condition.h, phasetype_amd/csrc/pht_condition.hip (no reference
# counterpart): which phase each unit still in service is in, its mean residual
# life, and the spares the fleet needs when failed units are replaced
CONDITION_MAX_H, CONDITION_MAX_UNITS, CONDITION_SCALE = 16, 1 << 22, 2.0 ** 40
CD_F_TRAP, CD_F_HCAP = 64, 128


def condition_finalise(words, scales, phisum, mrlsum, dsum, cnt, unit_index, flags, phi=None, mrl=None,
                       d=None) -> dict:
    """``Sweeper.condition``'s dict from the raw outputs (words int64 [draws,
    n + H + 3], scales [draws, 1 + H], phisum [units, n], mrlsum [units], dsum
    [units, H], cnt [units], the units' indices, the draws' flag words)."""
    words = np.asarray(words, np.int64)
    scales = np.asarray(scales, np.float64)
    phisum, mrlsum = np.asarray(phisum, np.float64), np.asarray(mrlsum, np.float64)
    dsum, cnt = np.asarray(dsum, np.float64), np.asarray(cnt, np.int64)
    n, H = phisum.shape[1], dsum.shape[1]
    k = np.maximum(cnt, 1).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        p_phase = np.where(cnt[:, None] > 0, phisum / k[:, None], np.nan)
        mrl_unit = np.where(cnt > 0, mrlsum / k, np.nan)
        demand_unit = np.where(cnt[:, None] > 0, dsum / k[:, None], np.nan)
    flags = np.asarray(flags, np.int32)
    out = dict(Phi=words[:, :n] / CONDITION_SCALE, L=(words[:, n] / CONDITION_SCALE) * scales[:, 0],
               Delta=(words[:, n + 1:n + 1 + H] / CONDITION_SCALE) * scales[:, 1:], nbad=words[:, n + H + 1].copy(),
               nunits=words[:, n + H + 2].copy(), words=words, scales=scales, phisum=phisum, mrlsum=mrlsum,
               dsum=dsum, cnt=cnt, p_phase=p_phase, mrl_unit=mrl_unit, demand_unit=demand_unit,
               unit_index=np.asarray(unit_index, np.int64), bad_draw=flags != 0, flags=flags)
    if phi is not None:
        out.update(phi=phi, mrl=mrl, d=d)
    return out


def condition_host(S, s, ages, horizons=None, ymax_c: float = 0.0, state=None) -> dict:
    """pht_condition_host (host only, no GPU): ``Sweeper.condition``'s dict for
    one draw over units of the given ``ages``, with the pointwise values; bit
    for bit what the device computes.  ``ymax_c``: the largest censored
    observation the tables are sized for (0: the largest age).  ``state``: the
    dict of the chain's earlier draws, whose per-unit sums and ``cnt`` this draw
    continues (its words are not kept)."""
    L = load()
    S = np.asarray(S, np.float64)
    n = S.shape[0]
    ages = np.ascontiguousarray(np.atleast_1d(ages), np.float64).reshape(-1)
    h = np.ascontiguousarray(np.atleast_1d([] if horizons is None else horizons), np.float64).reshape(-1)
    nc, H = len(ages), len(h)
    words, scales = np.zeros((1, n + H + 3), np.int64), np.zeros((1, 1 + H))
    if state is None:
        phisum, mrlsum, dsum, cnt = np.zeros((nc, n)), np.zeros(nc), np.zeros((nc, H)), np.zeros(nc, np.int64)
    else:
        phisum, mrlsum = np.array(state["phisum"], np.float64), np.array(state["mrlsum"], np.float64)
        dsum, cnt = np.array(state["dsum"], np.float64), np.array(state["cnt"], np.int64)
        if phisum.shape != (nc, n) or mrlsum.shape != (nc,) or dsum.shape != (nc, H) or cnt.shape != (nc,):
            raise ValueError("state does not have this call's units, states and horizons")
    phi, mrl, d = np.full((1, nc, n), np.nan), np.full((1, nc), np.nan), np.full((1, nc, H), np.nan)
    f = L.pht_condition_host(n, np.ascontiguousarray(S.reshape(-1, order="F")),
                             np.ascontiguousarray(s, np.float64).reshape(-1), nc, ages if nc else np.zeros(1), H,
                             h if H else np.zeros(1), float(ymax_c), words.reshape(-1), scales.reshape(-1),
                             phisum.ctypes.data, mrlsum.ctypes.data, dsum.ctypes.data if H else None,
                             cnt.ctypes.data, phi.ctypes.data, mrl.ctypes.data, d.ctypes.data if H else None)
    if f < 0:
        raise _err(L)
    return condition_finalise(words, scales, phisum, mrlsum, dsum, cnt, np.arange(nc), np.array([f], np.int32), phi,
                              mrl, d)


def condition_combine(a: dict, b: dict) -> dict:
    """The condition of two shards' units from the conditions of each
    (``Sweeper.condition`` of the same draws and horizons on each shard): the
    words add exactly (the scales depend on the draws alone), the per-unit
    blocks concatenate (``b``'s units after ``a``'s; ``unit_index`` stays each
    shard's own numbering)."""
    if a["words"].shape != b["words"].shape or not np.array_equal(a["flags"], b["flags"]) \
            or not np.array_equal(a["scales"], b["scales"]):
        raise ValueError("the two conditions are not of the same draws and horizons")
    pw = [np.concatenate([a[k], b[k]], axis=1) for k in ("phi", "mrl", "d")] if ("phi" in a and "phi" in b) \
        else [None] * 3
    return condition_finalise(a["words"] + b["words"], a["scales"], np.concatenate([a["phisum"], b["phisum"]]),
                              np.concatenate([a["mrlsum"], b["mrlsum"]]), np.concatenate([a["dsum"], b["dsum"]]),
                              np.concatenate([a["cnt"], b["cnt"]]),
                              np.concatenate([a["unit_index"], b["unit_index"]]), a["flags"], *pw)


def _draw_summary(x, use, band):
    """posterior mean, sd and quantiles over the rows of x [draws, ...] that count"""
    x = np.asarray(x, np.float64)
    sel = x[use]
    if not len(sel):
        nan = np.full(x.shape[1:], np.nan)
        return dict(mean=nan, sd=nan, band=np.full((len(band),) + x.shape[1:], np.nan))
    return dict(mean=sel.mean(0), sd=sel.std(0), band=np.quantile(sel, band, axis=0))


def fleet_condition(res, x, TT_or_T, censored, horizons=None, C_=None, n=None, burn: int = 0, thin: int = 1,
                    device: int = 0, batch: int = 64, collation: str = "C", band=(.025, .5, .975)) -> dict:
    """The condition of a fleet from a chain (``res`` and ``TT_or_T`` as in
    ``log_lik``; rows ``burn::thin``), for the units of ``x`` still in service
    (``censored`` != 0, at age x_i).  ``Sweeper.condition``'s dict, of which per
    unit ``p_phase`` [units, n] (the posterior law of the unit's phase: in a
    Coxian or birth-death structure, its wear stage), ``mrl_unit`` (its
    posterior mean residual life) and ``demand_unit`` [units, H] (its expected
    failures within each horizon when replaced at failure), plus ``stage``
    (argmax of p_phase, -1 where it is NaN) and, per draw and summarised over
    the ``n_used`` draws that are not flagged and have no bad unit, ``phase``
    (= Phi [draws, n], the fleet's composition), ``residual_life`` (= L, the
    fleet's total mean residual life) and ``demand`` (= Delta [draws, H], the
    spares needed with replacement), each with ``*_mean``, ``*_sd`` and
    ``*_band`` (the posterior ``band`` quantiles).  The demand of a draw is the
    MEAN of its replacement count: the variance of the count within a draw is
    not computed, so ``demand_sd`` is the spread between the draws only, a
    LOWER bound of the predictive sd (``fleet_spares`` gives both parts)."""
    S_list, s_list, n = _chain_draws(res, TT_or_T, C_, n, collation)
    S_list, s_list = S_list[int(burn)::int(thin)], s_list[int(burn)::int(thin)]
    if not S_list:
        raise ValueError("no rows left after burn / thin")
    sw = _obs_sweeper(x, censored, n, device)
    try:
        r = sw.condition(S_list, s_list, horizons, batch=batch)
    finally:
        sw.close()
    use = (~r["bad_draw"]) & (r["nbad"] == 0)
    r["use"], r["n_used"] = use, int(use.sum())
    with np.errstate(invalid="ignore"):
        r["stage"] = np.where(np.isnan(r["p_phase"]).any(1), -1, np.argmax(np.nan_to_num(r["p_phase"]), axis=1))
    for key, val in (("phase", r["Phi"]), ("residual_life", r["L"]), ("demand", r["Delta"])):
        sm = _draw_summary(val, use, band)
        r[key] = val
        r[key + "_mean"], r[key + "_sd"], r[key + "_band"] = sm["mean"], sm["sd"], sm["band"]
    r["horizons"] = np.atleast_1d(np.asarray([] if horizons is None else horizons, np.float64))
    return r


def _condition_one(S, s, t, horizons, device):
    S = np.asarray(S, np.float64)
    t = np.asarray(t, np.float64)
    sw = Sweeper(S.shape[0], METHODS["ECS"], 1, device=device)
    try:
        sw.set_obs(t.reshape(-1), np.ones(t.size, np.int32))
        r = sw.condition([S], [s], horizons, pointwise=True)
    finally:
        sw.close()
    if r["bad_draw"][0]:
        raise ValueError(f"not a usable generator (flag {r['flags'][0]})")
    return r, t


def ph_state(S, s, t, device: int = 0):
    """The law of the phase of PH(e_1, S) at ``t`` given survival to t:
    e_1 exp(S t) / (e_1 exp(S t) 1), [..., n] for a ``t`` of any shape
    (``Sweeper.condition`` on one draw; NaN beyond the evaluator's range)."""
    r, t = _condition_one(S, s, t, None, device)
    return r["phi"][0].reshape(t.shape + (r["phi"].shape[2],))


def ph_mrl(S, s, given=0.0, device: int = 0):
    """The mean residual life of PH(e_1, S) at age ``given`` (0: the mean):
    E[T - t | T > t], the shape of ``given``."""
    r, t = _condition_one(S, s, given, None, device)
    m = r["mrl"][0].reshape(t.shape)
    return float(m) if t.ndim == 0 else m


# --------------------------------------------------------------- fleet spares
# include/pht_spares.h, phasetype_amd/csrc/pht_spares.hip (no reference
# counterpart): the variance of the replacement count beside its mean, and the
# stock that covers the demand with a given probability
def spares_finalise(words, scales, dsum, vsum, d2sum, cnt, unit_index, flags, d=None, var=None) -> dict:
    """``Sweeper.spares``'s dict from the raw outputs (words int64 [draws,
    2 H + 2], scales [draws, 2 H], dsum, vsum, d2sum [units, H], cnt [units],
    the units' indices, the draws' flag words)."""
    words = np.asarray(words, np.int64)
    scales = np.asarray(scales, np.float64)
    dsum, vsum, d2sum = np.asarray(dsum, np.float64), np.asarray(vsum, np.float64), np.asarray(d2sum, np.float64)
    cnt = np.asarray(cnt, np.int64)
    H = dsum.shape[1]
    k = np.maximum(cnt, 1).astype(np.float64)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        demand_unit = np.where(cnt[:, None] > 0, dsum / k, np.nan)
        # the law of total variance per unit; a negative value is rounding alone
        sd = np.sqrt(np.maximum(vsum / k + d2sum / k - (dsum / k) ** 2, 0.0))
        demand_unit_sd = np.where(cnt[:, None] > 0, sd, np.nan)
    flags = np.asarray(flags, np.int32)
    out = dict(Delta=(words[:, :H] / CONDITION_SCALE) * scales[:, :H],
               V=(words[:, H:2 * H] / CONDITION_SCALE) * scales[:, H:], nbad=words[:, 2 * H].copy(),
               nunits=words[:, 2 * H + 1].copy(), words=words, scales=scales, dsum=dsum, vsum=vsum, d2sum=d2sum,
               cnt=cnt, demand_unit=demand_unit, demand_unit_sd=demand_unit_sd,
               unit_index=np.asarray(unit_index, np.int64), bad_draw=flags != 0, flags=flags)
    if d is not None:
        out.update(d=d, var=var)
    return out


def spares_host(S, s, ages, horizons, ymax_c: float = 0.0, state=None) -> dict:
    """pht_spares_host (host only, no GPU): ``Sweeper.spares``'s dict for one
    draw over units of the given ``ages``, with the pointwise values; bit for
    bit what the device computes.  ``ymax_c``: the largest censored observation
    the tables are sized for (0: the largest age).  ``state``: the dict of the
    chain's earlier draws, whose per-unit sums and ``cnt`` this draw continues
    (its words are not kept)."""
    L = load()
    S = np.asarray(S, np.float64)
    n = S.shape[0]
    ages = np.ascontiguousarray(np.atleast_1d(ages), np.float64).reshape(-1)
    h = np.ascontiguousarray(np.atleast_1d(horizons), np.float64).reshape(-1)
    nc, H = len(ages), len(h)
    words, scales = np.zeros((1, 2 * H + 2), np.int64), np.zeros((1, 2 * H))
    if state is None:
        dsum, vsum, d2sum, cnt = np.zeros((nc, H)), np.zeros((nc, H)), np.zeros((nc, H)), np.zeros(nc, np.int64)
    else:
        dsum, vsum = np.array(state["dsum"], np.float64), np.array(state["vsum"], np.float64)
        d2sum, cnt = np.array(state["d2sum"], np.float64), np.array(state["cnt"], np.int64)
        if dsum.shape != (nc, H) or vsum.shape != (nc, H) or d2sum.shape != (nc, H) or cnt.shape != (nc,):
            raise ValueError("state does not have this call's units and horizons")
    d, var = np.full((1, nc, H), np.nan), np.full((1, nc, H), np.nan)
    f = L.pht_spares_host(n, np.ascontiguousarray(S.reshape(-1, order="F")),
                          np.ascontiguousarray(s, np.float64).reshape(-1), nc, ages if nc else np.zeros(1), H,
                          h if H else np.zeros(1), float(ymax_c), words.reshape(-1),
                          scales.reshape(-1) if H else np.zeros(1), dsum.ctypes.data, vsum.ctypes.data,
                          d2sum.ctypes.data, cnt.ctypes.data, d.ctypes.data, var.ctypes.data)
    if f < 0:
        raise _err(L)
    return spares_finalise(words, scales, dsum, vsum, d2sum, cnt, np.arange(nc), np.array([f], np.int32), d, var)


def spares_combine(a: dict, b: dict) -> dict:
    """The spares of two shards' units from the spares of each
    (``Sweeper.spares`` of the same draws and horizons on each shard): the
    words add exactly (the scales depend on the draws alone; given the draw
    the units are independent, so their variances add as their means do), the
    per-unit blocks concatenate (``b``'s units after ``a``'s; ``unit_index``
    stays each shard's own numbering)."""
    if a["words"].shape != b["words"].shape or not np.array_equal(a["flags"], b["flags"]) \
            or not np.array_equal(a["scales"], b["scales"]):
        raise ValueError("the two spares results are not of the same draws and horizons")
    pw = [np.concatenate([a[k], b[k]], axis=1) for k in ("d", "var")] if ("d" in a and "d" in b) else [None] * 2
    return spares_finalise(a["words"] + b["words"], a["scales"], np.concatenate([a["dsum"], b["dsum"]]),
                           np.concatenate([a["vsum"], b["vsum"]]), np.concatenate([a["d2sum"], b["d2sum"]]),
                           np.concatenate([a["cnt"], b["cnt"]]),
                           np.concatenate([a["unit_index"], b["unit_index"]]), a["flags"], *pw)


def fleet_spares(res, x, TT_or_T, horizons, censored, C_=None, n=None, burn: int = 0, thin: int = 1,
                 device: int = 0, batch: int = 64, collation: str = "C") -> dict:
    """The spares a fleet needs from a chain (``res`` and ``TT_or_T`` as in
    ``log_lik``; rows ``burn::thin``; the arguments of ``fleet_forecast``): of
    the units of ``x`` still in service (``censored`` != 0, at age x_i), how
    many failures occur within each of ``horizons`` when every failed unit is
    replaced by a new one.  ``Sweeper.spares``'s dict plus, per horizon,
    ``mean`` (the expected number, ``fleet_condition``'s ``demand_mean``),
    ``sd`` (the predictive standard deviation by the law of total variance)
    with its two parts ``within`` = mean_d V_d (the count's own randomness
    given the parameters, which ``fleet_condition`` leaves out) and ``between``
    = var_d Delta_d (the posterior's: ``fleet_condition``'s ``demand_sd``
    squared), ``n_used`` (the draws that count: not flagged and with no bad
    unit) and ``stock(p)``: the smallest whole number of spares whose
    APPROXIMATE predictive probability of sufficing is at least p, the ceiling
    of ``forecast_count_quantiles(Delta, V, p)`` (the equal-weight mixture over
    the draws of normals matched to each draw's mean and variance; a count of
    few failures is skewed and discrete, which a normal is not)."""
    S_list, s_list, n = _chain_draws(res, TT_or_T, C_, n, collation)
    S_list, s_list = S_list[int(burn)::int(thin)], s_list[int(burn)::int(thin)]
    if not S_list:
        raise ValueError("no rows left after burn / thin")
    sw = _obs_sweeper(x, censored, n, device)
    try:
        r = sw.spares(S_list, s_list, horizons, batch=batch)
    finally:
        sw.close()
    use = np.broadcast_to(((~r["bad_draw"]) & (r["nbad"] == 0))[:, None], r["Delta"].shape)
    r.update(forecast_moments(r["Delta"], r["V"], use))
    Delta, V = r["Delta"], r["V"]
    r["use"] = use[:, 0].copy()
    r["stock"] = lambda p: np.ceil(forecast_count_quantiles(Delta, V, p, use))
    r["horizons"] = np.atleast_1d(np.asarray(horizons, np.float64))
    return r


def ph_renewal(S, s, h, given=0.0, device: int = 0):
    """(mean, variance) of the number of failures within ``h`` of one unit of
    age ``given`` (0: new) with law PH(e_1, S) that is replaced by a new one at
    every failure; each the shape of ``h`` (increasing where it has several
    values).  ``Sweeper.spares`` on one draw."""
    S = np.asarray(S, np.float64)
    hh = np.asarray(h, np.float64)
    sw = Sweeper(S.shape[0], METHODS["ECS"], 1, device=device)
    try:
        sw.set_obs(np.array([float(given)]), np.ones(1, np.int32))
        r = sw.spares([S], [s], hh.reshape(-1), pointwise=True)
    finally:
        sw.close()
    if r["bad_draw"][0]:
        raise ValueError(f"not a usable generator (flag {r['flags'][0]})")
    m, v = r["d"][0, 0].reshape(hh.shape), r["var"][0, 0].reshape(hh.shape)
    return (float(m), float(v)) if hh.ndim == 0 else (m, v)


# ------------------------------------------------- age-replacement policies
# include/pht_replace.h, phasetype_amd/csrc/pht_replace.hip (no reference
# counterpart): at what age to replace a unit preventively, and what it saves
RP_A_BEYOND, RP_A_EVAL, RP_A_DRAW = 1, 2, 4
RP_F_COST, RP_F_DRAW, RP_F_NOAGE, RP_F_UNREFINED, RP_F_EDGE, RP_F_EVAL, RP_F_NEVER, RP_F_CAP = \
    1, 2, 4, 8, 16, 32, 64, 128
REPLACE_MAX_AGES, REPLACE_MAX_PAIRS = 1024, 16


def replace_host(S, s, ages, cp, cf) -> dict:
    """pht_replace_host (host only, no GPU): ``Sweeper.replace``'s dict with the
    curve for one draw (policy arrays [P], curve arrays [G], ``m`` a float);
    bit for bit what the device computes."""
    L = load()
    S = np.asarray(S, np.float64)
    n = S.shape[0]
    ages = np.ascontiguousarray(np.atleast_1d(ages), np.float64).reshape(-1)
    cp = np.ascontiguousarray(np.atleast_1d(cp), np.float64).reshape(-1)
    cf = np.ascontiguousarray(np.atleast_1d(cf), np.float64).reshape(-1)
    if len(cp) != len(cf):
        raise ValueError("cp and cf must have the same length")
    G, P_ = len(ages), len(cp)
    out = dict(t=np.zeros(P_), g=np.zeros(P_), lo=np.zeros(P_), hi=np.zeros(P_), j=np.zeros(P_, np.int32),
               nev=np.zeros(P_, np.int32), flags=np.zeros(P_, np.uint32), lS=np.zeros(G), lf=np.zeros(G),
               M=np.zeros(G), age_flags=np.zeros(G, np.uint32))
    m = np.zeros(1)
    f = L.pht_replace_host(n, np.ascontiguousarray(S.reshape(-1, order="F")),
                           np.ascontiguousarray(s, np.float64).reshape(-1), G, ages, P_, cp, cf, out["t"], out["g"],
                           out["lo"], out["hi"], out["j"], out["nev"], out["flags"], m, out["lS"], out["lf"],
                           out["M"], out["age_flags"])
    if f < 0:
        raise _err(L)
    out.update(m=float(m[0]), bad_draw=f != 0, draw_flags=f)
    return out


def _mean_life(S) -> float:
    """E[T] of PH(e_1, S) with numpy (NaN where -S cannot be solved): only the
    default grid of ages is sized by it"""
    try:
        S = np.asarray(S, np.float64)
        return float(np.linalg.solve(-S, np.ones(S.shape[0]))[0])
    except np.linalg.LinAlgError:
        return float("nan")


def _default_ages(S_list) -> np.ndarray:
    """64 geometric ages from 0.02 to 8 times the median mean life of the draws"""
    m = np.array([_mean_life(S) for S in S_list])
    m = m[np.isfinite(m) & (m > 0)]
    if not len(m):
        raise ValueError("no draw has a finite mean life: give ages")
    return float(np.median(m)) * np.geomspace(0.02, 8.0, 64)


def age_replacement(S, s, cp, cf, ages=None, device: int = 0) -> dict:
    """The age-replacement policy of one law PH(e_1, S): ``Sweeper.replace`` on
    one draw with the curve, every array without the draws' axis (``cp``,
    ``cf`` scalars or [P]).  ``ages`` defaults to 64 geometric ages from 0.02
    to 8 mean lives."""
    S = np.asarray(S, np.float64)
    ages = _default_ages([S]) if ages is None else ages
    sw = Sweeper(S.shape[0], METHODS["ECS"], 1, device=device)
    try:
        r = sw.replace([S], [s], ages, cp, cf, pointwise=True)
    finally:
        sw.close()
    if r["bad_draw"][0]:
        raise ValueError(f"not a usable generator (flag {r['draw_flags'][0]})")
    out = {k: v[0] for k, v in r.items()}
    out["ages"] = np.atleast_1d(np.asarray(ages, np.float64))
    return out


def ph_rmean(S, s, tau, device: int = 0):
    """The restricted mean life E[min(T, tau)] of PH(e_1, S), the shape of
    ``tau`` (0 at tau = 0; NaN beyond 1400 / the largest rate).
    ``Sweeper.replace``'s curve on one draw."""
    S = np.asarray(S, np.float64)
    tt = np.asarray(tau, np.float64)
    flat = tt.reshape(-1)
    if not np.all(flat >= 0) or not np.all(np.isfinite(flat)):
        raise ValueError("tau must be finite and non-negative")
    out = np.zeros(flat.shape)
    ages, inv = np.unique(flat[flat > 0], return_inverse=True)
    if len(ages):
        sw = Sweeper(S.shape[0], METHODS["ECS"], 1, device=device)
        try:
            M = []
            for k in range(0, len(ages), REPLACE_MAX_AGES):
                r = sw.replace([S], [s], ages[k:k + REPLACE_MAX_AGES], 1.0, 2.0, pointwise=True)
                if r["bad_draw"][0]:
                    raise ValueError(f"not a usable generator (flag {r['draw_flags'][0]})")
                M.append(r["M"][0])
        finally:
            sw.close()
        out[flat > 0] = np.concatenate(M)[inv]
    out = out.reshape(tt.shape)
    return float(out) if tt.ndim == 0 else out


def replacement_summary(r: dict, ages, cp, cf, band=(.025, .5, .975)) -> dict:
    """The posterior summary of ``Sweeper.replace``'s dict with the curve (host
    arithmetic only): what ``ph_replacement`` returns."""
    ages = np.atleast_1d(np.asarray(ages, np.float64))
    cp, cf = np.atleast_1d(np.asarray(cp, np.float64)), np.atleast_1d(np.asarray(cf, np.float64))
    t, g, fl = r["t"], r["g"], r["flags"]
    nd, P_ = t.shape
    G = len(ages)
    flagged = np.isnan(t)
    never = ((fl & RP_F_NEVER) != 0) & ~flagged
    edge = ((fl & RP_F_EDGE) != 0) & ~never & ~flagged
    finite = ~flagged & ~never & ~edge
    ginf = cf[None, :] / r["m"][:, None]
    saving = 1.0 - g / ginf
    bands, sbands = np.full((len(band), P_), np.nan), np.full((len(band), P_), np.nan)
    for p in range(P_):
        fin = np.isfinite(t[:, p])
        if fin.any():
            bands[:, p] = np.quantile(t[fin, p], band)
        ok = ~np.isnan(saving[:, p])
        if ok.any():
            sbands[:, p] = np.quantile(saving[ok, p], band)
    # the posterior-mean cost curve over the ages at which every unflagged draw is good
    use = ~np.asarray(r["bad_draw"], bool)
    good_age = np.all(r["age_flags"][use] == 0, axis=0) if use.any() else np.zeros(G, bool)
    gbar = np.full((P_, G), np.nan)
    if use.any() and good_age.any():
        F = -np.expm1(r["lS"][use][:, good_age])
        M = r["M"][use][:, good_age]
        for p in range(P_):
            if 0 < cp[p] < cf[p] < np.inf:
                gbar[p, good_age] = ((cp[p] + (cf[p] - cp[p]) * F) / M).mean(0)
    age_bayes, g_bayes, evpi = np.full(P_, np.nan), np.full(P_, np.nan), np.full(P_, np.nan)
    for p in range(P_):
        if not np.all(np.isnan(gbar[p])):
            k = int(np.nanargmin(gbar[p]))
            age_bayes[p], g_bayes[p] = ages[k], gbar[p, k]
            ok = use & ~np.isnan(g[:, p])
            if ok.any():
                evpi[p] = g_bayes[p] - g[ok, p].mean()
    out = dict(r)
    out.update(ages=ages, cp=cp, cf=cf, band=bands, saving=saving, saving_band=sbands, n_finite=finite.sum(0),
               n_never=never.sum(0), n_edge=edge.sum(0), n_flagged=flagged.sum(0), g_inf=ginf, gbar=gbar,
               n_bad_ages=int((~good_age).sum()), age_bayes=age_bayes, g_bayes=g_bayes,
               g_inf_bar=ginf[use].mean(0) if use.any() else np.full(P_, np.nan), evpi=evpi)
    return out


def ph_replacement(res, TT_or_T, cp, cf, ages=None, C_=None, n=None, burn: int = 0, thin: int = 1, device: int = 0,
                   batch: int = 64, collation: str = "C", band=(.025, .5, .975)) -> dict:
    """Age-replacement policies of a chain (``res`` and ``TT_or_T`` as in
    ``log_lik``; rows ``burn::thin``; ``cp``, ``cf`` scalars or [P]).
    ``Sweeper.replace``'s dict with the curve plus, per cost pair: ``band``
    [len(band), P], the posterior ``band`` quantiles of the optimal age over
    its finite entries; ``n_finite`` (an interior optimum), ``n_never`` (running
    to failure costs no more: inf), ``n_edge`` (the cost rate still falls at the
    last age) and ``n_flagged`` (NaN), which sum to the draws; ``saving`` [draws,
    P] = 1 - g* / g_inf with ``saving_band``; ``gbar`` [P, G], the posterior
    mean of the cost curve over the ages at which every unflagged draw is good
    (NaN elsewhere, ``n_bad_ages`` of them); ``age_bayes`` [P], the argmin of
    ``gbar``: the age to choose under parameter uncertainty, with its cost rate
    ``g_bayes`` (compare ``g_inf_bar``, the mean cost rate of running to
    failure); ``evpi`` [P] = g_bayes - mean(g*), what knowing the parameters
    would save.  ``ages`` defaults to 64 geometric ages from 0.02 to 8 times
    the median mean life of the draws."""
    S_list, s_list, n = _chain_draws(res, TT_or_T, C_, n, collation)
    S_list, s_list = S_list[int(burn)::int(thin)], s_list[int(burn)::int(thin)]
    if not S_list:
        raise ValueError("no rows left after burn / thin")
    ages = _default_ages(S_list) if ages is None else ages
    sw = Sweeper(n, METHODS["ECS"], 1, device=device)
    try:
        r = sw.replace(S_list, s_list, ages, cp, cf, batch=batch, pointwise=True)
    finally:
        sw.close()
    return replacement_summary(r, ages, cp, cf, band)


def replacement_overdue(t, age_bayes, c, band=(.025, .5, .975)) -> dict:
    """Which units of ages ``c`` are past the optimal age (host arithmetic
    only): ``t`` [draws, P] the draws' optimal ages (inf: never; NaN: not
    usable), ``age_bayes`` [P].  Sorted ages and ``searchsorted``: no draws x
    units matrix."""
    t, c = np.asarray(t, np.float64), np.asarray(c, np.float64).reshape(-1)
    nd, P_ = t.shape
    cs = np.sort(c)
    p_over = np.full((P_, len(c)), np.nan)
    n_over = np.full((nd, P_), np.nan)
    nband = np.full((len(band), P_), np.nan)
    n_bayes = np.zeros(P_, np.int64)
    for p in range(P_):
        ok = ~np.isnan(t[:, p])
        if ok.any():
            ts = np.sort(t[ok, p])
            p_over[p] = np.searchsorted(ts, c, side="right") / float(ok.sum())
            n_over[ok, p] = len(c) - np.searchsorted(cs, t[ok, p], side="left")
            nband[:, p] = np.quantile(n_over[ok, p], band)
        n_bayes[p] = len(c) - np.searchsorted(cs, age_bayes[p], side="left") if not np.isnan(age_bayes[p]) else 0
    return dict(p_overdue=p_over, n_overdue=n_over, n_overdue_band=nband, n_overdue_bayes=n_bayes)


def fleet_replacement(res, x, TT_or_T, censored, cp, cf, ages=None, C_=None, n=None, burn: int = 0, thin: int = 1,
                      device: int = 0, batch: int = 64, collation: str = "C", band=(.025, .5, .975)) -> dict:
    """``ph_replacement`` applied to a fleet: of the units of ``x`` still in
    service (``censored`` != 0, at age x_i), ``p_overdue`` [P, units], the share
    of usable draws whose optimal age the unit has reached; ``n_overdue``
    [draws, P], the units past each draw's optimal age (NaN for an unusable
    draw) with ``n_overdue_band``; ``n_overdue_bayes`` [P], the units past
    ``age_bayes``; ``unit_index``, the units' positions in ``x``."""
    x = np.asarray(x, np.float64).reshape(-1)
    idx = np.nonzero(np.asarray(censored).reshape(-1) != 0)[0]
    if not len(idx):
        raise ValueError("no unit in service (censored != 0)")
    r = ph_replacement(res, TT_or_T, cp, cf, ages=ages, C_=C_, n=n, burn=burn, thin=thin, device=device, batch=batch,
                       collation=collation, band=band)
    r.update(replacement_overdue(r["t"], r["age_bayes"], x[idx], band))
    r["unit_index"] = idx
    return r


# ------------------------------------------- expected statistics, EM fitting
# include/pht_estep.h, phasetype_amd/csrc/pht_estep.hip (no reference
# counterpart): the exact conditional expectations of the statistics the
# sampler draws, and maximum-likelihood / MAP fitting by EM on top of them.
ESTEP_MAX_OBS = 1 << 22


def estep_contract(S, s, words, yscale):
    """pht_estep_contract (host only, no GPU): dict(Z [n], N [n, n], E [n],
    A [n], flag) of one draw from its int64 words (``Sweeper.estep``'s, of one shard
    or summed over shards that shared ``yscale``); bit for bit what the device
    computes."""
    L = load()
    S = np.asarray(S, np.float64)
    n = S.shape[0]
    words = np.ascontiguousarray(words, np.int64).reshape(-1)
    nw = L.pht_estep_words()
    if S.shape != (n, n) or not 1 <= n <= 32 or words.shape != (nw,):
        raise ValueError(f"need S [n, n] with 1 <= n <= 32 and {nw} words")
    Z, N, E, A = np.zeros(n), np.zeros(n * n), np.zeros(n), np.zeros(n)
    flag = L.pht_estep_contract(n, np.ascontiguousarray(S.reshape(-1, order="F")),
                                np.ascontiguousarray(s, np.float64), words, nw // 4 - 1, float(yscale), Z, N, E, A)
    if flag < 0:
        raise _err(L)
    return dict(Z=Z, N=N.reshape(n, n, order="F").copy(), E=E, A=A, flag=flag)


def complete_stats(S, s, Z, N, E, A):
    """The statistics of the COMPLETED paths from those on [0, y]: a censored
    observation's path goes on beyond y until absorption, which is what every
    sampler here draws for it (as the reference does) and sums into its
    statistics block.  From state occupancy A at the censoring times the rest
    of the path spends A (-S)^-1 in each state (-S is a non-singular M-matrix:
    a non-negative inverse), jumps at rate S_ij and exits at rate s_i from
    there.  Returns (Z, N, E) with that added; sum(E) is then the number of
    observations."""
    S = np.asarray(S, np.float64)
    after = np.linalg.solve(-S.T, np.asarray(A, np.float64))
    Zc = np.asarray(Z) + after
    Nc = np.asarray(N) + after[:, None] * (S - np.diag(np.diag(S)))
    return Zc, Nc, np.asarray(E) + after * np.asarray(s, np.float64)


def expected_stats(S, s, x, censored=None, device: int = 0, complete: bool = False) -> dict:
    """E[z | y], E[N | y], E[exits | y] of PH(e_1, S) with exit rates s, summed
    over the observations ``x`` / ``censored``: dict(Z [n], N [n, n], E [n],
    A [n], loglik, nbad) (Sweeper.estep of one draw).  By default on [0, y]
    (the likelihood's statistics: sum(Z) = sum(x), exits of exact observations
    only); ``complete``: of the completed paths (``complete_stats``), the
    expectation of what a sweep of an exact sampler sums."""
    S = np.asarray(S, np.float64)
    sw = _obs_sweeper(x, censored, S.shape[0], device)
    try:
        r = sw.estep([S], [s])
    finally:
        sw.close()
    Z, N, E, A = r["Z"][0], r["N"][0], r["E"][0], r["A"][0]
    if complete:
        Z, N, E = complete_stats(S, s, Z, N, E, A)
    return dict(Z=Z, N=N, E=E, A=A, loglik=float(r["loglik"][0]), nbad=int(r["nbad"][0]))


def em_step(T, C_, Z, N, E, prior=None) -> np.ndarray:
    """The M-step: per parameter p over its cells of T (numbers 1..m, 0 = a
    fixed zero), theta_p = sum Nt / sum C_cell Z_i with Nt = N_ij for a
    transient cell and E_i for the exit column: the likelihood's C Z, not the
    Gibbs update's z / C (they coincide at C = 1).  ``prior`` = (nu, zeta):
    the MAP step (nu - 1 + sum Nt) / (zeta + sum C Z) of the Gamma(nu, zeta)
    prior, floored at 1e-300."""
    T = np.asarray(T, np.int64)
    n = T.shape[0] - 1
    m = int(T.max())
    num, den = np.zeros(m), np.zeros(m)
    for i in range(n):
        for j in range(n + 1):
            p = int(T[i, j])
            if p == 0 or i == j:
                continue
            num[p - 1] += E[i] if j == n else N[i, j]
            den[p - 1] += C_[i, j] * Z[i]
    if prior is not None:
        num = num + np.asarray(prior[0], np.float64) - 1.0
        den = den + np.asarray(prior[1], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        theta = num / den
    return np.maximum(theta, 1e-300) if prior is not None else theta


def ph_em(x, TT_or_T, censored=None, C_=None, start=None, prior=None, iters: int = 200, tol: float = 1e-8,
          device: int = 0, collation: str = "C", estep=None) -> dict:
    """Maximum-likelihood (or, with ``prior`` = (nu, zeta) per parameter in
    phtMCMC2's order, MAP) fit of the structured phase-type model by EM, the
    E-step on the GPU over all of ``x`` / ``censored`` (Sweeper.estep).

    ``TT_or_T``, ``C_`` as in ``log_lik``; ``start``: the first theta (default:
    every rate 1 / mean(x)).  Stops after ``iters`` iterations or when the
    objective (log-likelihood, plus the log-prior for MAP) rises by less than
    ``tol`` (1 + |objective|).  Returns dict(theta (usable as ``start=`` of
    phtMCMC2 / Sweeper.gibbs), S, s, loglik (the trace: entry k is the
    log-likelihood at the theta BEFORE update k), objective, iterations,
    converged).  A generator that becomes flagged or non-finite, or an
    observation without density, ends the run with a PhaseTypeError.
    ``estep``: a callable (S, s) -> dict(Z, N, E, loglik) in place of the GPU
    (the tests drive the loop with the CPU restatement)."""
    T, names = _tt_numbers(TT_or_T, collation)
    n1 = T.shape[0]
    n, m = n1 - 1, int(T.max())
    C_ = np.ones((n1, n1)) if C_ is None else np.asarray(C_, np.float64)
    x = np.asarray(x, np.float64)
    theta = np.full(m, 1.0 / float(np.mean(x))) if start is None else np.array(start, np.float64).reshape(-1)
    if theta.shape != (m,):
        raise ValueError(f"start must hold {m} values")
    if prior is not None:
        prior = tuple(np.asarray([p[k] for k in names] if isinstance(p, dict) else p, np.float64) for p in prior)
    sw = None
    if estep is None:
        sw = _obs_sweeper(x, censored, n, device)

        def estep(S, s):
            r = sw.estep([S], [s])
            if int(r["flags"][0]) != 0:
                raise PhaseTypeError(f"ph_em: the generator is not usable (flag {int(r['flags'][0])})")
            return dict(Z=r["Z"][0], N=r["N"][0], E=r["E"][0], loglik=float(r["loglik"][0]))
    trace, objective, converged, it = [], [], False, 0
    try:
        for it in range(1, int(iters) + 1):
            if not np.all(np.isfinite(theta)):
                raise PhaseTypeError(f"ph_em: a non-finite rate at iteration {it}")
            S, s = theta_to_S(theta, T, C_)
            r = estep(S, s)
            ll = float(r["loglik"])
            if not np.isfinite(ll):
                raise PhaseTypeError(f"ph_em: log-likelihood {ll} at iteration {it} (a bad observation or an "
                                     "unusable generator)")
            obj = ll
            if prior is not None:
                obj = ll + float(np.sum((prior[0] - 1.0) * np.log(theta) - prior[1] * theta))
            trace.append(ll)
            objective.append(obj)
            if len(objective) > 1 and abs(obj - objective[-2]) < tol * (1.0 + abs(obj)):
                converged = True
                break
            theta = em_step(T, C_, r["Z"], r["N"], r["E"], prior)
    finally:
        if sw is not None:
            sw.close()
    S, s = theta_to_S(theta, T, C_)
    return dict(theta=theta, S=S, s=s, loglik=np.array(trace), objective=np.array(objective), iterations=it,
                converged=converged, vars=names)


# ------------------------------------------------------------- PSIS-LOO
# include/pht_psis.h, phasetype_amd/csrc/pht_psis.hip (no reference
# counterpart); everything below Sweeper.psis_loo is numpy.
PSIS_MAX_DRAWS = 16384


def loo_from_psis(r: dict) -> dict:
    """The summary of a Sweeper.psis_loo result (or of several shards'
    results with their per-observation arrays concatenated)."""
    elpd_i, p_i, khat = np.asarray(r["elpd_i"]), np.asarray(r["p_loo_i"]), np.asarray(r["khat"])
    N, S = len(elpd_i), int(r["n_draws_used"])
    elpd = float(np.sum(elpd_i))
    thr = min(1.0 - 1.0 / np.log10(S), 0.7) if S > 1 else 0.0
    return dict(elpd_loo=elpd, p_loo=float(np.sum(p_i)), looic=-2.0 * elpd,
                se_elpd_loo=float(np.sqrt(N * np.var(elpd_i))), lppd=float(np.sum(r["lppd_i"])),
                pointwise=(elpd_i, p_i, khat), khat_threshold=float(thr), n_khat_above=int(np.sum(khat > thr)),
                n_draws_used=S)


def loo(res, x, TT_or_T=None, censored=None, C_=None, n=None, burn: int = 0, thin: int = 1, device: int = 0,
        batch: int = 64, collation: str = "C", evaluator: str = "spectral") -> dict:
    """PSIS-LOO cross-validation of a chain (rows ``burn::thin``) over data
    ``x`` / ``censored`` (Sweeper.psis_loo): dict(elpd_loo, p_loo, looic,
    se_elpd_loo = sqrt(N var(elpd_i)), lppd, pointwise=(elpd_i, p_loo_i,
    khat), khat_threshold = min(1 - 1 / log10(S), 0.7), n_khat_above,
    n_draws_used).  An observation with khat above the threshold is one whose
    leave-one-out density these draws cannot estimate; WAIC is off there too,
    silently.  At most 16384 draws after thinning, and draws x observations x
    8 bytes must fit the device: thin further otherwise."""
    S_list, s_list, n = _chain_draws(res, TT_or_T, C_, n, collation)
    S_list, s_list = S_list[int(burn)::int(thin)], s_list[int(burn)::int(thin)]
    sw = _obs_sweeper(x, censored, n, device)
    try:
        return loo_from_psis(sw.psis_loo(S_list, s_list, batch=batch, evaluator=evaluator))
    finally:
        sw.close()


def loo_compare(a: dict, b: dict) -> dict:
    """Two ``loo`` results on the same data: dict(elpd_diff = elpd_a - elpd_b,
    se_diff = sqrt(N var(elpd_i^a - elpd_i^b))).  numpy only."""
    ea, eb = np.asarray(a["pointwise"][0], np.float64), np.asarray(b["pointwise"][0], np.float64)
    if ea.shape != eb.shape:
        raise ValueError(f"the two results cover {ea.shape} and {eb.shape} observations: not the same data")
    d = ea - eb
    return dict(elpd_diff=float(np.sum(d)), se_diff=float(np.sqrt(len(d) * np.var(d))))


# ------------------------------------------------- posterior-predictive checks
# include/pht_predict.h, phasetype_amd/csrc/pht_predict.hip (no reference
# counterpart): replicated absorption times of PH(e_1, S_d) for posterior
# draws, reduced exactly on the GPU; everything below the kernel call is numpy.
PRED_WORDS = 8  # int64 words per draw: [Hy, Fy, Hq, Fq, ndone, nbad, nsurv, njump]
PRED_MAX_REP = 1 << 22  # replicates per draw and call
PRED_MAX_EDGES = 1024
PRED_MAX_JUMPS = 1 << 20
PRED_F_RATE, PRED_F_ABSORB = 16, 32  # flag words next to LL_F_NONFINITE, LL_F_MU (pht_predict.h)


def pred_table(S, s):
    """One draw's table (pht_pred_build; host only): (flag, scale [n],
    cum [n, n]), the per-row running sums of the jump probabilities over the
    candidates k != j in increasing k, the exit last, +inf from the last
    candidate of positive probability on.  A flagged draw's table is zero."""
    L = load()
    S = np.asarray(S, np.float64)
    n = S.shape[0]
    words = L.pht_pred_table_words(n)
    if words < 0 or S.shape != (n, n):
        raise ValueError(f"S must be square with 1 <= n <= 32, got {S.shape}")
    tab = np.zeros(words)
    flag = L.pht_pred_build(n, np.ascontiguousarray(S.reshape(-1, order="F")),
                            np.ascontiguousarray(s, np.float64).reshape(-1), tab, words)
    if flag < 0:
        raise _err(L)
    return flag, tab[:n].copy(), tab[n:].reshape(n, n).copy()


def predict_finalise(words, counts, ymin, ymax, flags, edges) -> dict:
    """``Sweeper.predict``'s dict from the (summed) integer words and counts,
    the (min / max combined) extremes, the flag words and the edges."""
    words = np.asarray(words, np.int64).reshape(-1, PRED_WORDS)
    nd = words.shape[0]
    edges = np.asarray(edges, np.float64).reshape(-1)
    counts = np.asarray(counts, np.int64).reshape(nd, len(edges) + 1)
    flags = np.asarray(flags, np.int32).reshape(nd)
    ndone = words[:, 4].astype(np.float64)
    sy = words[:, 0].astype(np.float64) + words[:, 1].astype(np.float64) * 2.0 ** -32
    sq = words[:, 2].astype(np.float64) + words[:, 3].astype(np.float64) * 2.0 ** -32
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(ndone > 0, sy / ndone, np.nan)
        var = np.where(ndone > 1, (sq - sy * sy / ndone) / (ndone - 1.0), np.nan)
        ecdf = np.where(ndone[:, None] > 0, np.cumsum(counts[:, :-1], axis=1) / ndone[:, None], np.nan)
    some = ndone > 0
    return dict(mean=mean, var=var, ymin=np.where(some, np.asarray(ymin, np.float64), np.nan),
                ymax=np.where(some, np.asarray(ymax, np.float64), np.nan), ndone=words[:, 4].copy(),
                nbad=words[:, 5].copy(), nsurv=words[:, 6].copy(), njump=words[:, 7].copy(), counts=counts,
                ecdf=ecdf, words=words, bad_draw=flags != 0, flags=flags, edges=edges)


def predict_combine(a: dict, b: dict) -> dict:
    """Two ``predict`` results of the same draws and edges over disjoint
    replicate ranges, as one: words and counts add, ymin / ymax combine by
    min / max, pointwise values are joined in the order (a, b)."""
    if a["words"].shape != b["words"].shape or not np.array_equal(a["edges"], b["edges"]):
        raise ValueError("the two results must cover the same draws with the same edges")
    if not np.array_equal(a["flags"], b["flags"]):
        raise ValueError("the two results flag different draws")
    out = predict_finalise(a["words"] + b["words"], a["counts"] + b["counts"],
                           np.fmin(a["ymin"], b["ymin"]), np.fmax(a["ymax"], b["ymax"]), a["flags"], a["edges"])
    if "y" in a and "y" in b:
        out["y"] = np.concatenate([a["y"], b["y"]], axis=1)
        out["jumps"] = np.concatenate([a["jumps"], b["jumps"]], axis=1)
    return out


def _predict_chunks(sw, S_list, s_list, nrep, **kw):
    """sw.predict over nrep replicates in calls of at most 2^22, by rep0"""
    out, rep0 = None, int(kw.pop("rep0", 0))
    nrep = int(nrep)
    if nrep < 1:
        raise ValueError("nrep must be at least 1")
    for lo in range(0, nrep, PRED_MAX_REP):
        r = sw.predict(S_list, s_list, min(PRED_MAX_REP, nrep - lo), rep0=rep0 + lo, **kw)
        out = r if out is None else predict_combine(out, r)
    return out


def rph(S, s, N: int, key=(1, 2), device: int = 0) -> np.ndarray:
    """N variates of PH(e_1, S) (absorption times of the chain started in
    state 1), simulated on the GPU: variate i is replicate i of draw 0 under
    ``key``, whatever N is.  NaN where a path exceeded 2^20 jumps or 2^20."""
    S = np.asarray(S, np.float64)
    sw = Sweeper(S.shape[0], METHODS["ECS"], 1, device=device)
    try:
        r = _predict_chunks(sw, [S], [s], N, key=key, pointwise=True)
        if r["bad_draw"][0]:
            raise ValueError(f"not a phase-type generator with certain absorption from state 1 (flag {r['flags'][0]})")
        return r["y"][0]
    finally:
        sw.close()


def posterior_predictive(res, TT_or_T, nrep: int, edges=None, C_=None, n=None, burn: int = 0, thin: int = 1,
                         key=(1, 2), horizon: float = np.inf, device: int = 0, batch: int = 64,
                         collation: str = "C") -> dict:
    """``Sweeper.predict`` over the rows ``burn::thin`` of a chain (``res`` and
    ``TT_or_T`` as in ``log_lik``): ``nrep`` replicated absorption times per
    row, their moments, extremes and histogram on ``edges``.  Row k of the
    selection is draw number k of the streams."""
    S_list, s_list, n = _chain_draws(res, TT_or_T, C_, n, collation)
    S_list, s_list = S_list[int(burn)::int(thin)], s_list[int(burn)::int(thin)]
    if not S_list:
        raise ValueError("no rows left after burn / thin")
    sw = Sweeper(n, METHODS["ECS"], 1, device=device)
    try:
        return _predict_chunks(sw, S_list, s_list, nrep, key=key, edges=edges, horizon=horizon, batch=batch)
    finally:
        sw.close()


def quantiles_from_counts(counts, edges, ymin, ymax, q) -> np.ndarray:
    """Quantiles [draws, len(q)] of histogrammed values: ``counts``
    [draws, ne + 1] over ``edges`` (bin = the number of edges <= y), the
    outer bins closed by ymin / ymax; linear within the bin that holds the
    rank q * total (the histogram's resolution: exact at an edge)."""
    counts = np.atleast_2d(np.asarray(counts, np.float64))
    edges = np.asarray(edges, np.float64).reshape(-1)
    q = np.atleast_1d(np.asarray(q, np.float64))
    nd = counts.shape[0]
    lo = np.concatenate([np.asarray(ymin, np.float64).reshape(nd, 1), np.broadcast_to(edges, (nd, len(edges)))], axis=1)
    hi = np.concatenate([np.broadcast_to(edges, (nd, len(edges))), np.asarray(ymax, np.float64).reshape(nd, 1)], axis=1)
    lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)  # (an extreme inside a neighbouring bin's range)
    cum = np.cumsum(counts, axis=1)
    out = np.full((nd, len(q)), np.nan)
    for d in range(nd):
        tot = cum[d, -1]
        if not tot > 0:
            continue
        for i, qq in enumerate(q):
            rank = qq * tot
            b = min(int(np.searchsorted(cum[d], rank, "left")), counts.shape[1] - 1)
            below = cum[d, b - 1] if b > 0 else 0.0
            frac = (rank - below) / counts[d, b] if counts[d, b] > 0 else 0.0
            out[d, i] = lo[d, b] + frac * (hi[d, b] - lo[d, b])
    return out


def _ppc_data(x, censored, horizon):
    """(x as recorded, horizon or inf): exact data, or administratively
    censored at ``horizon`` (every censored observation equals it)"""
    x = np.asarray(x, np.float64).reshape(-1)
    if len(x) < 2:
        raise ValueError("need at least two observations")
    cen = np.zeros(len(x), bool) if censored is None else np.asarray(censored).reshape(-1) != 0
    if len(cen) != len(x):
        raise ValueError("censored must have the data's length")
    if cen.any():
        if horizon is None:
            raise ValueError("ppc compares exact data; censored observations need `horizon` (administrative "
                             "censoring: every censored observation equals it)")
        if not np.all(x[cen] == float(horizon)) or np.any(x[~cen] > float(horizon)):
            raise ValueError("with `horizon`, every censored observation must equal it and no exact one exceed it")
    return x, (np.inf if horizon is None else float(horizon))


def ppc_from_predict(pred: dict, x, quantiles=(.05, .25, .5, .75, .95)) -> dict:
    """The numpy finalisation of ``ppc``: ``pred`` a ``predict`` result whose
    edges are the sorted distinct values of the data ``x`` (as recorded).

    Per usable draw (not flagged, some replicate recorded) the test
    quantities T(y_rep) — mean, sd, min, max from the exact words, the
    quantiles from the histogram (``quantiles_from_counts``) — against T(x);
    ``p[name]`` = mean(T(y_rep) >= T(x)) over those draws.  ``band``: the
    2.5 / 50 / 97.5 % of ``ecdf`` over the draws at each edge, ``ecdf_x`` the
    data's share below each edge (the same convention)."""
    x = np.asarray(x, np.float64).reshape(-1)
    use = (~np.asarray(pred["bad_draw"], bool)) & (np.asarray(pred["ndone"]) > 1)
    edges = np.asarray(pred["edges"], np.float64)
    qs = tuple(float(v) for v in quantiles)
    qrep = quantiles_from_counts(pred["counts"], edges, pred["ymin"], pred["ymax"], qs)
    T_rep = dict(mean=pred["mean"], sd=np.sqrt(pred["var"]), min=pred["ymin"], max=pred["ymax"])
    T_x = dict(mean=float(np.mean(x)), sd=float(np.std(x, ddof=1)), min=float(np.min(x)), max=float(np.max(x)))
    for i, v in enumerate(qs):
        T_rep[f"q{v:g}"] = qrep[:, i]
        T_x[f"q{v:g}"] = float(np.quantile(x, v))
    T_rep = {k: np.asarray(v, np.float64) for k, v in T_rep.items()}
    p = {k: (float(np.mean(T_rep[k][use] >= T_x[k])) if use.any() else np.nan) for k in T_rep}
    out = dict(p=p, T_x=T_x, T_rep=T_rep, n_draws_used=int(use.sum()), edges=edges,
               ecdf_x=np.array([np.mean(x < e) for e in edges]))
    out["band"] = (np.quantile(pred["ecdf"][use], [.025, .5, .975], axis=0) if use.any()
                   else np.full((3, len(edges)), np.nan))
    return out


def ppc(res, x, TT_or_T=None, nrep=None, censored=None, horizon=None, quantiles=(.05, .25, .5, .75, .95), C_=None,
        n=None, burn: int = 0, thin: int = 1, key=(1, 2), device: int = 0, batch: int = 64,
        collation: str = "C") -> dict:
    """Posterior predictive check of a chain against data ``x``: for every row
    (``burn::thin``) ``nrep`` (default len(x)) replicates on the GPU
    (``posterior_predictive``), histogrammed on the data's sorted distinct
    values (thinned evenly to 1024 edges where there are more), then
    ``ppc_from_predict``.  Exact data only; with ``censored``, ``horizon``
    must be given and every censored observation equal it (administrative
    censoring): data and replicates are then both compared as recorded at the
    horizon.  Returns ``ppc_from_predict``'s dict plus ``predict``."""
    x, hz = _ppc_data(x, censored, horizon)
    edges = np.unique(x)
    if len(edges) > PRED_MAX_EDGES:
        edges = edges[np.unique(np.round(np.linspace(0, len(edges) - 1, PRED_MAX_EDGES)).astype(np.int64))]
    pred = posterior_predictive(res, TT_or_T, len(x) if nrep is None else int(nrep), edges=edges, C_=C_, n=n,
                                burn=burn, thin=thin, key=key, horizon=hz, device=device, batch=batch,
                                collation=collation)
    out = ppc_from_predict(pred, x, quantiles)
    out["predict"] = pred
    return out
