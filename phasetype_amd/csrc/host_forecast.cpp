/*
 * host_forecast.cpp — fleet forecasts: the conditional failure probability of
 * every censored unit of the context at every horizon for every draw
 * (specification: include/pht_forecast.h; kernel: pht_forecast.hip, the tables
 * by pht_loglik_unif.hip's table kernel).  No reference counterpart.
 * pht_ctx_forecast runs draws x censored units x (horizons + 1) evaluations
 * on the device over the context's resident observations; pht_forecast_host
 * is the specification's function for one draw on the host (no device).
 */
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <numeric>

#include "host_internal.h"
#include "pht_forecast.h"
#include "pht_forecast_args.h"
#include "pht_loglik_unif_args.h"

using namespace pht;
using namespace pht::host;

namespace {

/* what both entry points refuse about the horizons */
bool horizons_ok(const char *who, int nh, const double *h) {
  if (nh < 1 || nh > PHT_FC_MAXH || !h) {
    set_err("%s: need 1 <= nh <= %d horizons", who, PHT_FC_MAXH);
    return false;
  }
  if (!pht_fc_horizons_ok(nh, h)) {
    set_err("%s: every horizon must be finite, >= 0 and larger than the one before", who);
    return false;
  }
  return true;
}

/* the censored units of the context's observations, listed once per
 * pht_ctx_set_obs: ages in the device order, the caller's index and rank */
int forecast_units(pht_ctx *c, const char *who) {
  if (!c) {
    set_err("%s: null context", who);
    return -1;
  }
  auto &fc = c->obs.fc;
  if (fc.ncens >= 0) return 0;
  if (c->count < 1 || !c->obs.d_y) {
    fc.ncens = 0;
    return 0;
  }
  HIPCHK(hipSetDevice(c->device));
  ctx_drain(c);
  std::vector<int> cens((size_t)c->count);
  HIPCHK(hipMemcpy(cens.data(), c->obs.d_cens.get(), sizeof(int) * (size_t)c->count, hipMemcpyDeviceToHost));
  std::vector<double> ages;
  fc.idx.clear();
  fc.ymax_c = 0.0;
  for (long k = 0; k < c->count; k++) {
    if (!cens[k]) continue;
    ages.push_back(c->h_ysorted[k]);
    fc.idx.push_back(c->order[k]);
    fc.ymax_c = std::max(fc.ymax_c, c->h_ysorted[k]);
  }
  const long nc = (long)ages.size();
  std::vector<long> by(nc);
  std::iota(by.begin(), by.end(), 0L);
  std::sort(by.begin(), by.end(), [&](long x, long y) { return fc.idx[x] < fc.idx[y]; });
  fc.rank.assign(nc, 0);
  for (long r = 0; r < nc; r++) fc.rank[by[r]] = r;
  if (nc > 0 && nc <= PHT_FC_MAXUNITS) {
    HIPCHK(fc.d_age.alloc((size_t)nc));
    HIPCHK(hipMemcpy(fc.d_age.get(), ages.data(), sizeof(double) * (size_t)nc, hipMemcpyHostToDevice));
  }
  fc.ncens = nc;
  return 0;
}

}  // namespace

extern "C" int pht_forecast_host(int n, const double *S, const double *s, long ncens, const double *ages, int nh,
                                 const double *horizons, double ymax_c, long long *words_out, double *qsum,
                                 long long *cnt, double *q_out) {
  if (n < 1 || n > kMaxN || !S || !s || !ages || !words_out) {
    set_err("pht_forecast_host: need 1 <= n <= %d, S, s, ages and words_out", kMaxN);
    return -1;
  }
  if (ncens < 1) {
    set_err("pht_forecast_host: no censored unit (ncens >= 1)");
    return -1;
  }
  if (ncens > PHT_FC_MAXUNITS) {
    set_err("pht_forecast_host: %ld censored units, at most %ld (the int64 sums)", ncens, (long)PHT_FC_MAXUNITS);
    return -1;
  }
  if (!horizons_ok("pht_forecast_host", nh, horizons)) return -1;
  double amax = 0.0;
  for (long i = 0; i < ncens; i++) amax = (ages[i] > amax) ? ages[i] : amax;
  if (ymax_c != 0.0 && !(ymax_c >= amax && ymax_c < INFINITY)) {
    set_err("pht_forecast_host: ymax_c must be 0 (the largest age) or finite and at least the largest age");
    return -1;
  }
  std::vector<double> tab(3 * (size_t)(PHT_LLU_MAXK + 1));
  return (int)pht_fc_draw(n, S, s, ncens, ages, ymax_c != 0.0 ? ymax_c : amax, nh, horizons, tab.data(),
                          tab.data() + 2 * (PHT_LLU_MAXK + 1), words_out, qsum, cnt, q_out);
}

extern "C" long pht_ctx_forecast_units(pht_ctx *c, long *idx_out) {
  if (forecast_units(c, "pht_ctx_forecast_units")) return -1;
  const auto &fc = c->obs.fc;
  if (idx_out)
    for (long u = 0; u < fc.ncens; u++) idx_out[fc.rank[u]] = fc.idx[u];
  return fc.ncens;
}

extern "C" int pht_ctx_forecast_grid_cap(pht_ctx *c, int cap) {
  if (!c || cap < 0) {
    set_err("pht_ctx_forecast_grid_cap: need a context and cap >= 0 (0: the default)");
    return -1;
  }
  c->fc_grid_cap = cap;
  return 0;
}

extern "C" int pht_ctx_forecast_ms(pht_ctx *c, float *table_ms, float *eval_ms) {
  if (!c) {
    set_err("pht_ctx_forecast_ms: null context");
    return -1;
  }
  if (table_ms) *table_ms = c->fc_ms[0];
  if (eval_ms) *eval_ms = c->fc_ms[1];
  return 0;
}

extern "C" int pht_ctx_forecast(pht_ctx *c, int ndraws, const double *S, const double *s, int nh,
                                const double *horizons, int batch, long long *words_out, double *qsum_out,
                                long long *cnt_out, double *q_out, int *draw_flags_out) {
  if (forecast_units(c, "pht_ctx_forecast")) return -1;
  auto &fc = c->obs.fc;
  if (fc.ncens < 1) {
    set_err("pht_ctx_forecast: no censored observation on this context (pht_ctx_set_obs)");
    return -1;
  }
  if (fc.ncens > PHT_FC_MAXUNITS) {
    set_err("pht_ctx_forecast: %ld censored units on this context, at most %ld (the int64 sums): shard them",
            fc.ncens, (long)PHT_FC_MAXUNITS);
    return -1;
  }
  if (!horizons_ok("pht_ctx_forecast", nh, horizons)) return -1;
  if (ndraws < 1 || !S || !s || !words_out || !qsum_out || !cnt_out || batch < 1 || batch > kLoglikBatch) {
    set_err("pht_ctx_forecast: need ndraws >= 1, S, s, words_out, qsum_out, cnt_out and 1 <= batch <= %d",
            kLoglikBatch);
    return -1;
  }
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream.get();
  ctx_drain(c);
  const int n = c->n;
  const long nc = fc.ncens;
  for (auto &e : c->fc_ev)
    if (!e) HIPCHK(e.create());
  int grid_cap = c->fc_grid_cap;
  if (!grid_cap) { /* under 80 KB of LDS a block: two blocks a CU */
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    grid_cap = std::max(1, cus) * 2;
  }

  /* the draws' meta words: K for the largest age plus the last horizon */
  const double ymax = pht_fc_ymax(fc.ymax_c, horizons[nh - 1]);
  std::vector<double> meta((size_t)ndraws * PHT_LLU_META);
  int Kcall = 0;
  for (int d = 0; d < ndraws; d++) {
    double *m = meta.data() + (size_t)d * PHT_LLU_META;
    const unsigned flag = pht_llu_meta(n, S + (size_t)d * n * n, s + (size_t)d * n, ymax, m);
    if (draw_flags_out) draw_flags_out[d] = (int)flag;
    Kcall = std::max(Kcall, (int)m[PHT_LLU_M_K]);
  }
  const int stride = 2 * (Kcall + 1);
  const int bmax = std::min(batch, ndraws);
  /* the device keeps slots >= nh state words a unit (the kernel's build for few or many horizons) */
  const int slots = pht_fcast_slots(nh);
  const size_t nS = (size_t)ndraws * n * n, ns = (size_t)ndraws * n, cells = (size_t)nc * nh;
  const size_t scells = (size_t)nc * slots;
  const size_t nwords = (size_t)ndraws * nh * PHT_FC_WORDS;
  HIPCHK(ensure(c->d_lluin, c->lluin_cap, nS + ns + meta.size()));
  HIPCHK(ensure(c->d_llutab, c->llutab_cap, (size_t)bmax * stride));
  HIPCHK(ensure(c->d_fch, c->fch_cap, (size_t)PHT_FC_MAXH));
  HIPCHK(ensure(c->d_fcwords, c->fcwords_cap, nwords));
  HIPCHK(ensure(fc.d_qsum, fc.qsum_cap, scells));
  HIPCHK(ensure(fc.d_cnt, fc.cnt_cap, scells));
  if (q_out) HIPCHK(ensure(fc.d_q, fc.q_cap, (size_t)bmax * cells));
  double *dS = c->d_lluin.get(), *ds = dS + nS, *dmeta = ds + ns;
  HIPCHK(hipMemcpyAsync(dS, S, sizeof(double) * nS, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(ds, s, sizeof(double) * ns, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dmeta, meta.data(), sizeof(double) * meta.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->d_fch.get(), horizons, sizeof(double) * nh, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(c->d_fcwords.get(), 0, sizeof(unsigned long long) * nwords, st));
  HIPCHK(hipMemsetAsync(fc.d_qsum.get(), 0, sizeof(double) * scells, st));
  HIPCHK(hipMemsetAsync(fc.d_cnt.get(), 0, sizeof(int) * scells, st));
  std::vector<double> hq;
  if (q_out) hq.resize((size_t)bmax * cells);
  c->fc_ms[0] = c->fc_ms[1] = 0.f;
  for (int d0 = 0; d0 < ndraws; d0 += batch) {
    const int nb = std::min(batch, ndraws - d0);
    int Kmax = 0;
    for (int d = d0; d < d0 + nb; d++) Kmax = std::max(Kmax, (int)meta[(size_t)d * PHT_LLU_META + PHT_LLU_M_K]);
    HIPCHK(hipEventRecord(c->fc_ev[0].get(), st));
    LlunifTableArgs t{};
    t.n = n;
    t.nd = nb;
    t.S = dS + (size_t)d0 * n * n;
    t.s = ds + (size_t)d0 * n;
    t.meta = dmeta + (size_t)d0 * PHT_LLU_META;
    t.tab = c->d_llutab.get();
    t.stride = stride;
    HIPCHK(pht_launch_llunif_table(&t, st));
    HIPCHK(hipEventRecord(c->fc_ev[1].get(), st));
    FcastArgs a{};
    a.nd = nb;
    a.nh = nh;
    a.Kmax = Kmax;
    a.count = nc;
    a.age = fc.d_age.get();
    a.meta = t.meta;
    a.tab = t.tab;
    a.stride = stride;
    a.h = c->d_fch.get();
    a.words = c->d_fcwords.get() + (size_t)d0 * nh * PHT_FC_WORDS;
    a.qsum = fc.d_qsum.get();
    a.cnt = fc.d_cnt.get();
    a.q = q_out ? fc.d_q.get() : nullptr;
    HIPCHK(pht_launch_fcast(&a, grid_cap, st));
    HIPCHK(hipEventRecord(c->fc_ev[2].get(), st));
    if (q_out)
      HIPCHK(hipMemcpyAsync(hq.data(), fc.d_q.get(), sizeof(double) * (size_t)nb * cells, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms0 = 0.f, ms1 = 0.f;
    HIPCHK(hipEventElapsedTime(&ms0, c->fc_ev[0].get(), c->fc_ev[1].get()));
    HIPCHK(hipEventElapsedTime(&ms1, c->fc_ev[1].get(), c->fc_ev[2].get()));
    c->fc_ms[0] += ms0;
    c->fc_ms[1] += ms1;
    if (q_out) { /* back into the caller's order of the censored observations */
      for (int d = 0; d < nb; d++) {
        const double *src = hq.data() + (size_t)d * cells;
        double *dst = q_out + (size_t)(d0 + d) * cells;
        for (long u = 0; u < nc; u++) memcpy(dst + (size_t)fc.rank[u] * nh, src + (size_t)u * nh, sizeof(double) * nh);
      }
    }
  }
  c->last_ms = c->fc_ms[0] + c->fc_ms[1];
  std::vector<double> hs(scells);
  std::vector<int> hc(scells);
  HIPCHK(hipMemcpyAsync(words_out, c->d_fcwords.get(), sizeof(long long) * nwords, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hs.data(), fc.d_qsum.get(), sizeof(double) * scells, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hc.data(), fc.d_cnt.get(), sizeof(int) * scells, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  /* every unit of an evaluated draw is good or bad: nunits = ncens - nbad */
  for (int d = 0; d < ndraws; d++) {
    if (pht_d2u(meta[(size_t)d * PHT_LLU_META + PHT_LLU_M_FLAG]) != 0) continue;
    for (int j = 0; j < nh; j++) {
      long long *w = words_out + ((size_t)d * nh + j) * PHT_FC_WORDS;
      w[PHT_FC_W_NUNITS] = (long long)nc - w[PHT_FC_W_NBAD];
    }
  }
  for (long u = 0; u < nc; u++) {
    const size_t dst = (size_t)fc.rank[u] * nh, src = (size_t)u * slots;
    for (int j = 0; j < nh; j++) {
      qsum_out[dst + j] = hs[src + j];
      cnt_out[dst + j] = hc[src + j];
    }
  }
  return 0;
}
