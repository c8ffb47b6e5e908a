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
  if (!c || cap < 0) {
    set_err("pht_ctx_estep_grid_cap: null context or negative cap");
    return -1;
  }
  c->es_grid_cap = cap;
  return 0;
}

extern "C" int pht_ctx_estep_ms(pht_ctx *c, float *hist_ms, float *contract_ms) {
  if (!c) {
    set_err("pht_ctx_estep_ms: null context");
    return -1;
  }
  if (hist_ms) *hist_ms = c->es_ms[0];
  if (contract_ms) *contract_ms = c->es_ms[1];
  return 0;
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
  if (!c->ll_grid_cap) {
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    c->ll_grid_cap = std::max(1, cus) * 4;
  }
  /* one block a CU (its LDS), unless the caller caps the grid */
  const int grid_cap = c->es_grid_cap > 0 ? c->es_grid_cap : std::max(1, c->ll_grid_cap / 4);
  for (auto &e : c->es_ev)
    if (!e) HIPCHK(e.create());

  std::vector<double> meta((size_t)ndraws * PHT_LLU_META);
  int Kcall = 0;
  for (int d = 0; d < ndraws; d++) {
    double *m = meta.data() + (size_t)d * PHT_LLU_META;
    const unsigned flag = pht_llu_meta(n, S + (size_t)d * n * n, s + (size_t)d * n, c->ymax, m);
    if (flags_out) flags_out[d] = (int)flag;
    Kcall = std::max(Kcall, (int)m[PHT_LLU_M_K]);
  }
  const int stride = 2 * (Kcall + 1);
  const int bmax = std::min(batch, ndraws);
  const size_t nS = (size_t)ndraws * n * n, ns = (size_t)ndraws * n;
  HIPCHK(ensure(c->d_lluin, c->lluin_cap, nS + ns + meta.size()));
  HIPCHK(ensure(c->d_llutab, c->llutab_cap, (size_t)bmax * stride));
  HIPCHK(ensure(c->d_lltot, c->lltot_cap, (size_t)ndraws * PHT_LL_TOT));
  HIPCHK(ensure(c->d_eswords, c->eswords_cap, (size_t)bmax * PHT_ES_WORDS));
  if (contract) HIPCHK(ensure(c->d_esout, c->esout_cap, (size_t)bmax * no));
  double *dS = c->d_lluin.get(), *ds = dS + nS, *dmeta = ds + ns;
  HIPCHK(hipMemcpyAsync(dS, S, sizeof(double) * nS, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(ds, s, sizeof(double) * ns, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dmeta, meta.data(), sizeof(double) * meta.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(c->d_lltot.get(), 0, sizeof(unsigned long long) * (size_t)ndraws * PHT_LL_TOT, st));
  std::vector<double> hout(contract ? (size_t)bmax * no : 0);
  c->es_ms[0] = c->es_ms[1] = 0.f;
  for (int d0 = 0; d0 < ndraws; d0 += batch) {
    const int nb = std::min(batch, ndraws - d0);
    int Kmax = 0;
    for (int d = d0; d < d0 + nb; d++) Kmax = std::max(Kmax, (int)meta[(size_t)d * PHT_LLU_META + PHT_LLU_M_K]);
    HIPCHK(hipMemsetAsync(c->d_eswords.get(), 0, sizeof(long long) * (size_t)nb * PHT_ES_WORDS, st));
    HIPCHK(hipEventRecord(c->es_ev[0].get(), st));
    LlunifTableArgs t{};
    t.n = n;
    t.nd = nb;
    t.S = dS + (size_t)d0 * n * n;
    t.s = ds + (size_t)d0 * n;
    t.meta = dmeta + (size_t)d0 * PHT_LLU_META;
    t.tab = c->d_llutab.get();
    t.stride = stride;
    HIPCHK(pht_launch_llunif_table(&t, st));
    EstepHistArgs a{};
    a.nd = nb;
    a.Kmax = Kmax;
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
    HIPCHK(hipEventRecord(c->es_ev[1].get(), st));
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
    HIPCHK(hipEventRecord(c->es_ev[2].get(), st));
    if (contract)
      HIPCHK(hipMemcpyAsync(hout.data(), c->d_esout.get(), sizeof(double) * (size_t)nb * no, hipMemcpyDeviceToHost,
                            st));
    if (words)
      HIPCHK(hipMemcpyAsync(words + (size_t)d0 * PHT_ES_WORDS, c->d_eswords.get(),
                            sizeof(long long) * (size_t)nb * PHT_ES_WORDS, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms0 = 0.f, ms1 = 0.f;
    HIPCHK(hipEventElapsedTime(&ms0, c->es_ev[0].get(), c->es_ev[1].get()));
    HIPCHK(hipEventElapsedTime(&ms1, c->es_ev[1].get(), c->es_ev[2].get()));
    c->es_ms[0] += ms0;
    c->es_ms[1] += ms1;
    for (int d = 0; contract && d < nb; d++) {
      const double *o = hout.data() + (size_t)d * no;
      memcpy(Z + (size_t)(d0 + d) * n, o, sizeof(double) * n);
      memcpy(N + (size_t)(d0 + d) * n * n, o + n, sizeof(double) * n * n);
      memcpy(E + (size_t)(d0 + d) * n, o + n + n * n, sizeof(double) * n);
      memcpy(A + (size_t)(d0 + d) * n, o + 2 * n + n * n, sizeof(double) * n);
    }
  }
  c->last_ms = c->es_ms[0] + c->es_ms[1];
  HIPCHK(hipMemcpyAsync(totals, c->d_lltot.get(), sizeof(long long) * (size_t)ndraws * PHT_LL_TOT,
                        hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}
