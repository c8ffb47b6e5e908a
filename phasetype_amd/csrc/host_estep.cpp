/*
 * host_estep.cpp — the expected sufficient statistics (E-step) of draws or EM
 * iterates over a shard's resident observations (specification:
 * include/pht_estep.h; kernels: pht_estep.hip, the tables by
 * pht_loglik_unif.hip's table kernel).  No reference counterpart.
 * pht_ctx_estep runs the histograms and, where asked, the contraction on the
 * device; pht_estep_contract is the specification's contraction on the host
 * (no device), for callers that sum the words of several shards first.
 */
#include <math.h>
#include <string.h>

#include <cmath>

#include "host_internal.h"
#include "pht_estep.h"
#include "pht_estep_args.h"
#include "pht_loglik_unif_args.h"

using namespace pht;
using namespace pht::host;

extern "C" int pht_estep_words(void) { return PHT_ES_WORDS; }

extern "C" double pht_estep_yscale(double ymax) { return pht_es_yscale(ymax); }

extern "C" int pht_estep_contract(int n, const double *S, const double *s, const long long *words, int K,
                                  double yscale, double *Z, double *N, double *E, double *A) {
  if (n < 1 || n > kMaxN || !S || !s || !words || !Z || !N || !E || !A || K < 0 || K > PHT_LLU_MAXK) {
    set_err("pht_estep_contract: need 1 <= n <= %d, 0 <= K <= %d and no null argument", kMaxN, PHT_LLU_MAXK);
    return -1;
  }
  if (!pht_es_yscale_ok(yscale)) {
    set_err("pht_estep_contract: yscale must be a positive finite power of two");
    return -1;
  }
  return (int)pht_es_contract(n, S, s, words, K, yscale, Z, N, E, A);
}

extern "C" int pht_ctx_estep_grid_cap(pht_ctx *c, int cap) {
  return grid_cap_set("pht_ctx_estep_grid_cap", "null context or negative cap", c, &pht_ctx::es_grid_cap, cap);
}

extern "C" int pht_ctx_estep_ms(pht_ctx *c, float *hist_ms, float *contract_ms) {
  return clock_read("pht_ctx_estep_ms", c, &pht_ctx::es_clk, hist_ms, contract_ms);
}

extern "C" int pht_ctx_estep(pht_ctx *c, int ndraws, const double *S, const double *s, int batch, double yscale,
                             long long *totals, long long *words, double *Z, double *N, double *E, double *A,
                             int *flags_out) {
  if (!c) {
    set_err("pht_ctx_estep: null context");
    return -1;
  }
  if (c->count < 1 || !c->obs.d_y) {
    set_err("pht_ctx_estep: no observations set on this context (pht_ctx_set_obs)");
    return -1;
  }
  if (ndraws < 1 || !S || !s || !totals || batch < 1 || batch > kLoglikBatch) {
    set_err("pht_ctx_estep: need ndraws >= 1, S, s, totals and 1 <= batch <= %d", kLoglikBatch);
    return -1;
  }
  const bool contract = Z || N || E || A;
  if (contract && !(Z && N && E && A)) {
    set_err("pht_ctx_estep: Z, N, E and A are given together or not at all");
    return -1;
  }
  const long long all = std::max<long long>(c->count, c->global_count);
  if (all > PHT_ES_MAXOBS) {
    set_err("pht_ctx_estep: %lld observations in all shards, at most %ld (the int64 words' range)", all,
            (long)PHT_ES_MAXOBS);
    return -1;
  }
  if (!(yscale > 0.0)) yscale = pht_es_yscale(c->ymax);
  if (!pht_es_yscale_ok(yscale) || yscale < c->ymax) {
    set_err("pht_ctx_estep: yscale must be a power of two >= the largest observation (%g)", c->ymax);
    return -1;
  }
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream.get();
  ctx_drain(c);
  const int n = c->n, no = n * n + 3 * n;
  /* one block a CU (its LDS), unless the caller caps the grid */
  const int grid_cap = c->es_grid_cap > 0 ? c->es_grid_cap : cu_count(c);
  if (grid_cap < 0) return -1;

  const UnifPlan plan(n, ndraws, S, s, batch, flags_out, [&](int, const double *Sd, const double *sd, double *m) {
    return pht_llu_meta(n, Sd, sd, c->ymax, m);
  });
  const int bmax = plan.bmax, stride = plan.stride;
  if (unif_stage(c, plan, S, s)) return -1;
  HIPCHK(ensure(c->d_lltot, (size_t)ndraws * PHT_LL_TOT));
  HIPCHK(ensure(c->d_eswords, (size_t)bmax * PHT_ES_WORDS));
  if (contract) HIPCHK(ensure(c->d_esout, (size_t)bmax * no));
  HIPCHK(hipMemsetAsync(c->d_lltot.get(), 0, sizeof(unsigned long long) * (size_t)ndraws * PHT_LL_TOT, st));
  std::vector<double> hout(contract ? (size_t)bmax * no : 0);
  PhaseClock &clk = c->es_clk;
  if (clk.begin()) return -1;
  for (int d0 = 0; d0 < ndraws; d0 += batch) {
    const int nb = std::min(batch, ndraws - d0);
    HIPCHK(hipMemsetAsync(c->d_eswords.get(), 0, sizeof(long long) * (size_t)nb * PHT_ES_WORDS, st));
    if (clk.mark(0, st)) return -1;
    LlunifTableArgs t;
    if (unif_tables(c, plan, d0, nb, t)) return -1;
    EstepHistArgs a{};
    a.nd = nb;
    a.Kmax = plan.Kmax(d0, nb);
    a.count = c->count;
    a.y = c->obs.d_y.get();
    a.cens = c->obs.d_cens.get();
    a.meta = t.meta;
    a.tab = t.tab;
    a.stride = stride;
    a.ryscale = 1.0 / yscale;
    a.totals = c->d_lltot.get() + (size_t)d0 * PHT_LL_TOT;
    a.words = reinterpret_cast<unsigned long long *>(c->d_eswords.get());
    HIPCHK(pht_launch_estep_hist(&a, grid_cap, st));
    if (clk.mark(1, st)) return -1;
    if (contract) {
      EstepContractArgs k{};
      k.n = n;
      k.nd = nb;
      k.S = t.S;
      k.s = t.s;
      k.meta = t.meta;
      k.tab = t.tab;
      k.stride = stride;
      k.words = c->d_eswords.get();
      k.yscale = yscale;
      k.out = c->d_esout.get();
      HIPCHK(pht_launch_estep_contract(&k, st));
    }
    if (clk.mark(2, st)) return -1;
    if (contract)
      HIPCHK(hipMemcpyAsync(hout.data(), c->d_esout.get(), sizeof(double) * (size_t)nb * no, hipMemcpyDeviceToHost,
                            st));
    if (words)
      HIPCHK(hipMemcpyAsync(words + (size_t)d0 * PHT_ES_WORDS, c->d_eswords.get(),
                            sizeof(long long) * (size_t)nb * PHT_ES_WORDS, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (clk.add_after_sync()) return -1;
    for (int d = 0; contract && d < nb; d++) {
      const double *o = hout.data() + (size_t)d * no;
      memcpy(Z + (size_t)(d0 + d) * n, o, sizeof(double) * n);
      memcpy(N + (size_t)(d0 + d) * n * n, o + n, sizeof(double) * n * n);
      memcpy(E + (size_t)(d0 + d) * n, o + n + n * n, sizeof(double) * n);
      memcpy(A + (size_t)(d0 + d) * n, o + 2 * n + n * n, sizeof(double) * n);
    }
  }
  c->last_ms = clk.total();
  HIPCHK(hipMemcpyAsync(totals, c->d_lltot.get(), sizeof(long long) * (size_t)ndraws * PHT_LL_TOT,
                        hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}
