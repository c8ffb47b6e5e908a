/*
 * host_r.cpp — the host runtime's face towards R and its error text.
 *
 *  - LJMA_Gibbs: the reference's .C entry point (src/PHT_MCMC_Aslett.c:104,
 *    registered by src/Registrations.c:6-20), re-implemented: the Gibbs
 *    bookkeeping and conjugate Gamma update stay on the host exactly as in
 *    src/PHT_MCMC_Aslett.c:187-405 (host_gibbs.cpp); step 1 (the
 *    per-observation latent-path sampling, :276-337) runs as HIP kernels on
 *    every visible GPU, each GPU owning a contiguous shard of the
 *    observations, and the integer sufficient statistics are summed on the
 *    host (exact, order-free).
 *  - R_init_PhaseType: registers LJMA_Gibbs for `.C` when loaded by R.
 *  - pht_last_error and the R-compatible stream of the pht_* C ABI
 *    (include/phasetype_amd.h; the other units hold the rest of it).
 *
 * Random numbers: inside R, R's own unif_rand/rgamma (resolved at run time);
 * standalone, the R-compatible stream of rstream.c.  Per-observation draws
 * on the device come from Philox keyed by two R-stream uniforms drawn at
 * LJMA_Gibbs entry (pht_philox.h).
 */
#include <dlfcn.h>
#include <stdarg.h>
#include <stdio.h>

#include "host_internal.h"

using namespace pht;
using namespace pht::host;

/* ======================================================= error reporting */
thread_local std::string pht::host::g_err;
void pht::host::set_err(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
}
extern "C" const char *pht_last_error(void) { return g_err.c_str(); }

/* ================================================ R runtime (when inside R) */
RHost::RHost() {
  unif = (unif_fn)dlsym(RTLD_DEFAULT, "unif_rand");
  rgamma = (rgamma_fn)dlsym(RTLD_DEFAULT, "rgamma");
  getrng = (void_fn)dlsym(RTLD_DEFAULT, "GetRNGstate");
  putrng = (void_fn)dlsym(RTLD_DEFAULT, "PutRNGstate");
  rprintf = (printf_fn)dlsym(RTLD_DEFAULT, "Rprintf");
  rerror = (error_fn)dlsym(RTLD_DEFAULT, "Rf_error");
  flush = (void_fn)dlsym(RTLD_DEFAULT, "R_FlushConsole");
  inR = unif && rgamma && getrng && putrng && rprintf && !getenv("PHT_STANDALONE_RNG");
  pht_rs_set_seed(&rs, 1234u);
}
RHost &pht::host::rhost() {
  static RHost h;
  return h;
}
static int g_verbose = 0;
/* Rprintf inside R; otherwise to `out`, if anywhere */
static void emit(const char *fmt, va_list ap, FILE *out) {
  RHost &h = rhost();
  char buf[512];
  vsnprintf(buf, sizeof buf, fmt, ap);
  if (h.inR) {
    h.rprintf("%s", buf);
    if (h.flush) h.flush();
  } else if (out) {
    fputs(buf, out);
    fflush(out);
  }
}
void pht::host::say(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  emit(fmt, ap, g_verbose ? stdout : nullptr);
  va_end(ap);
}
void pht::host::warn(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  emit(fmt, ap, stderr);
  va_end(ap);
}

extern "C" void pht_set_seed(uint32_t seed) { pht_rs_set_seed(&rhost().rs, seed); }
extern "C" double pht_unif_rand(void) { return rhost().u(); }
extern "C" double pht_rgamma(double a, double scale) { return rhost().gamma(a, scale); }
extern "C" void pht_set_verbose(int v) { g_verbose = v; }
extern "C" int pht_in_R(void) { return rhost().inR ? 1 : 0; }

/* ======================================================= .C entry point */
/*
 * Drop-in replacement of LJMA_Gibbs (src/PHT_MCMC_Aslett.c:104): same 15
 * arguments, same semantics and output (res[iter + i*it]).  Observations are
 * sharded over all visible GPUs (PHT_DEVICES=k limits the count).
 * Divergences, documented in DESIGN.md: per-observation draws come from
 * Philox (keyed by two R-stream uniforms drawn at entry) instead of R's
 * serial stream; z is reduced in exact fixed point.
 */
extern "C" void LJMA_Gibbs(int *it, int *mhit, int *method, int *n, int *m, double *nu, double *zeta, int *T,
                           double *C, double *y, int *l, int *censored, double *start, int *silent, double *res) {
  RHost &R = rhost();
  g_err.clear();
  R.begin();
  const uint32_t k0 = (uint32_t)(R.u() * 4294967296.0);
  const uint32_t k1 = (uint32_t)(R.u() * 4294967296.0);
  const int zexp = pht_zexp(y, *l);
  say("Setting up Gibbs run ...\n");
  int ndev = pht_device_count();
  ndev = std::min(ndev, env_int("PHT_DEVICES", ndev));
  /* PHT_CTX_PER_DEVICE=k: k shards (contexts, each with its own streams) per
   * device; the chain is the same for every k (tests/test_gpu_edges.py) */
  const int per = std::max(1, std::min(16, env_int("PHT_CTX_PER_DEVICE", 1)));
  std::vector<pht_ctx *> ctxs;
  int rc = 0;
  if (ndev <= 0) {
    set_err("no HIP device available");
    rc = -1;
  }
  const long L = *l;
  const int nsh = ndev * per;
  for (int d = 0; d < nsh && rc == 0; d++) {
    const long lo = L * d / nsh, hi = L * (d + 1) / nsh;
    pht_ctx *c = pht_ctx_create(d / per, *n, *method, *mhit);
    if (!c) {
      rc = -1;
      break;
    }
    ctxs.push_back(c);
    if (pht_ctx_set_obs(c, y + lo, censored + lo, hi - lo, lo)) rc = -1;
  }
  if (rc == 0)
    rc = gibbs_run(R, *it, *method, *n, *m, nu, zeta, T, C, *silent, start, res, ctxs, k0, k1, zexp, nullptr, nullptr,
                   nullptr);
  for (pht_ctx *c : ctxs) pht_ctx_destroy(c);
  if (rc == 0) say("\n\nCompleted MCMC run, returning results ...\n");
  R.end();
  if (rc != 0) {
    if (R.inR && R.rerror) R.rerror("%s", g_err.c_str());
    fprintf(stderr, "PhaseType (MI355X): %s\n", g_err.c_str());
  }
}

/* ================================================== R native registration */
/* R's registration ABI (R_ext/Rdynload.h), declared here so the library
 * also loads outside R; the R functions are resolved only when present. */
extern "C" {
typedef void *(*pht_DL_FUNC)(void);
typedef unsigned int pht_R_NativePrimitiveArgType;
typedef struct {
  const char *name;
  pht_DL_FUNC fun;
  int numArgs;
  pht_R_NativePrimitiveArgType *types;
} pht_R_CMethodDef;
}

extern "C" void R_init_PhaseType(void *dll) {
  /* INTSXP = 13, REALSXP = 14 (src/Registrations.c:6-9) */
  static pht_R_NativePrimitiveArgType types[15] = {13, 13, 13, 13, 13, 14, 14, 13, 14, 14, 13, 13, 14, 13, 14};
  static pht_R_CMethodDef cMethods[] = {{"LJMA_Gibbs", (pht_DL_FUNC)&LJMA_Gibbs, 15, types},
                                        {nullptr, nullptr, 0, nullptr}};
  typedef int (*reg_fn)(void *, const pht_R_CMethodDef *, const void *, const void *, const void *);
  typedef int (*bool_fn)(void *, int);
  reg_fn reg = (reg_fn)dlsym(RTLD_DEFAULT, "R_registerRoutines");
  bool_fn dyn = (bool_fn)dlsym(RTLD_DEFAULT, "R_useDynamicSymbols");
  bool_fn force = (bool_fn)dlsym(RTLD_DEFAULT, "R_forceSymbols");
  if (!reg || !dyn || !force) return;
  reg(dll, cMethods, nullptr, nullptr, nullptr);
  dyn(dll, 0);
  force(dll, 1);
}
