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

#include "host_internal.h"
#include "pht_forecast.h"
#include "pht_forecast_args.h"
#include "pht_loglik_unif_args.h"

using namespace pht;
using namespace pht::host;

extern "C" int pht_forecast_host(int n, const double *S, const double *s, long ncens, const double *ages, int nh,
                                 const double *horizons, double ymax_c, long long *words_out, double *qsum,
                                 long long *cnt, double *q_out) {
  if (n < 1 || n > kMaxN || !S || !s || !ages || !words_out) {
    set_err("pht_forecast_host: need 1 <= n <= %d, S, s, ages and words_out", kMaxN);
    return -1;
  }
  const char *who = "pht_forecast_host";
  double ymax = 0.0;
  if (!units_ok(who, ncens, PHT_FC_MAXUNITS) || !horizons_ok(who, nh, horizons, 1, PHT_FC_MAXH, pht_fc_horizons_ok) ||
      !ymax_c_ok(who, ncens, ages, ymax_c, &ymax))
    return -1;
  std::vector<double> tab(3 * (size_t)(PHT_LLU_MAXK + 1));
  return (int)pht_fc_draw(n, S, s, ncens, ages, ymax, nh, horizons, tab.data(), tab.data() + 2 * (PHT_LLU_MAXK + 1),
                          words_out, qsum, cnt, q_out);
}

extern "C" int pht_ctx_forecast_grid_cap(pht_ctx *c, int cap) {
  return grid_cap_set("pht_ctx_forecast_grid_cap", "need a context and cap >= 0 (0: the default)", c,
                      &pht_ctx::fc_grid_cap, cap);
}

extern "C" int pht_ctx_forecast_ms(pht_ctx *c, float *table_ms, float *eval_ms) {
  return clock_read("pht_ctx_forecast_ms", c, &pht_ctx::fc_clk, table_ms, eval_ms);
}

extern "C" int pht_ctx_forecast(pht_ctx *c, int ndraws, const double *S, const double *s, int nh,
                                const double *horizons, int batch, long long *words_out, double *qsum_out,
                                long long *cnt_out, double *q_out, int *draw_flags_out) {
  if (censored_units(c, "pht_ctx_forecast", PHT_FC_MAXUNITS)) return -1;
  auto &fc = c->obs.fc;
  if (!horizons_ok("pht_ctx_forecast", nh, horizons, 1, PHT_FC_MAXH, pht_fc_horizons_ok)) return -1;
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
  /* under 80 KB of LDS a block: two blocks a CU */
  const int grid_cap = c->fc_grid_cap ? c->fc_grid_cap : 2 * cu_count(c);
  if (grid_cap < 0) return -1;

  /* the draws' meta words: K for the largest age plus the last horizon */
  const double ymax = pht_fc_ymax(fc.ymax_c, horizons[nh - 1]);
  const UnifPlan plan(n, ndraws, S, s, batch, draw_flags_out, [&](int, const double *Sd, const double *sd, double *m) {
    return pht_llu_meta(n, Sd, sd, ymax, m);
  });
  const int bmax = plan.bmax;
  /* the device keeps slots >= nh state words a unit (the kernel's build for few or many horizons) */
  const int slots = pht_fcast_slots(nh);
  const size_t cells = (size_t)nc * nh, scells = (size_t)nc * slots;
  const size_t nwords = (size_t)ndraws * nh * PHT_FC_WORDS;
  if (unif_stage(c, plan, S, s)) return -1;
  HIPCHK(ensure(c->d_fch, (size_t)PHT_FC_MAXH));
  HIPCHK(ensure(c->d_fcwords, nwords));
  HIPCHK(ensure(fc.d_qsum, scells));
  HIPCHK(ensure(fc.d_cnt, scells));
  if (q_out) HIPCHK(ensure(fc.d_q, (size_t)bmax * cells));
  HIPCHK(hipMemcpyAsync(c->d_fch.get(), horizons, sizeof(double) * nh, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(c->d_fcwords.get(), 0, sizeof(unsigned long long) * nwords, st));
  HIPCHK(hipMemsetAsync(fc.d_qsum.get(), 0, sizeof(double) * scells, st));
  HIPCHK(hipMemsetAsync(fc.d_cnt.get(), 0, sizeof(int) * scells, st));
  std::vector<double> hq;
  if (q_out) hq.resize((size_t)bmax * cells);
  PhaseClock &clk = c->fc_clk;
  if (clk.begin()) return -1;
  for (int d0 = 0; d0 < ndraws; d0 += batch) {
    const int nb = std::min(batch, ndraws - d0);
    if (clk.mark(0, st)) return -1;
    LlunifTableArgs t;
    if (unif_tables(c, plan, d0, nb, t)) return -1;
    if (clk.mark(1, st)) return -1;
    FcastArgs a{};
    a.nd = nb;
    a.nh = nh;
    a.Kmax = plan.Kmax(d0, nb);
    a.count = nc;
    a.age = fc.d_age.get();
    a.meta = t.meta;
    a.tab = t.tab;
    a.stride = t.stride;
    a.h = c->d_fch.get();
    a.words = c->d_fcwords.get() + (size_t)d0 * nh * PHT_FC_WORDS;
    a.qsum = fc.d_qsum.get();
    a.cnt = fc.d_cnt.get();
    a.q = q_out ? fc.d_q.get() : nullptr;
    HIPCHK(pht_launch_fcast(&a, grid_cap, st));
    if (clk.mark(2, st)) return -1;
    if (q_out)
      HIPCHK(hipMemcpyAsync(hq.data(), fc.d_q.get(), sizeof(double) * (size_t)nb * cells, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (clk.add_after_sync()) return -1;
    if (q_out) { /* back into the caller's order of the censored observations */
      for (int d = 0; d < nb; d++) {
        const double *src = hq.data() + (size_t)d * cells;
        double *dst = q_out + (size_t)(d0 + d) * cells;
        for (long u = 0; u < nc; u++) memcpy(dst + (size_t)fc.rank[u] * nh, src + (size_t)u * nh, sizeof(double) * nh);
      }
    }
  }
  c->last_ms = clk.total();
  std::vector<double> hs(scells);
  std::vector<int> hc(scells);
  HIPCHK(hipMemcpyAsync(words_out, c->d_fcwords.get(), sizeof(long long) * nwords, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hs.data(), fc.d_qsum.get(), sizeof(double) * scells, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hc.data(), fc.d_cnt.get(), sizeof(int) * scells, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  /* every unit of an evaluated draw is good or bad: nunits = ncens - nbad */
  for (int d = 0; d < ndraws; d++) {
    if (plan.flagged(d)) continue;
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
