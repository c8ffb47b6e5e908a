/*
 * host_spares.cpp — fleet spares: the mean and the variance of the failures
 * with replacement of every censored unit of the context for every draw and
 * horizon (specification: include/pht_spares.h; kernels: pht_spares.hip, the
 * (ax, ac) tables by pht_loglik_unif.hip's table kernel, the forward tables by
 * pht_condition.hip's).  No reference counterpart.  pht_ctx_spares runs draws x
 * censored units windows on the device over the context's resident
 * observations; the draws' moment vectors r_h, q_h and scales are built on the
 * device too, the host decides the flags only (pht_sp_flags: nothing with a Kr
 * factor).  pht_spares_host is the specification's function for one draw on
 * the host (no device).
 */
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include "host_internal.h"
#include "pht_loglik_unif_args.h"
#include "pht_spares.h"
#include "pht_spares_args.h"

using namespace pht;
using namespace pht::host;

extern "C" int pht_spares_host(int n, const double *S, const double *s, long ncens, const double *ages, int nh,
                               const double *horizons, double ymax_c, long long *words_out, double *scales_out,
                               double *dsum, double *vsum, double *d2sum, long long *cnt, double *d_out,
                               double *var_out) {
  if (n < 1 || n > kMaxN || !S || !s || !ages || !words_out || !scales_out) {
    set_err("pht_spares_host: need 1 <= n <= %d, S, s, ages, words_out and scales_out", kMaxN);
    return -1;
  }
  const char *who = "pht_spares_host";
  double ymax = 0.0;
  if (!units_ok(who, ncens, PHT_CD_MAXUNITS) || !horizons_ok(who, nh, horizons, 1, PHT_CD_MAXH, pht_sp_horizons_ok) ||
      !ymax_c_ok(who, ncens, ages, ymax_c, &ymax))
    return -1;
  std::vector<double> work(PHT_SP_WORK(n, nh));
  return (int)pht_sp_draw(n, S, s, ncens, ages, ymax, nh, horizons, work.data(), words_out, scales_out, dsum, vsum,
                          d2sum, cnt, d_out, var_out);
}

extern "C" int pht_ctx_spares_grid_cap(pht_ctx *c, int cap) {
  return grid_cap_set("pht_ctx_spares_grid_cap", "need a context and cap >= 0 (0: the default)", c,
                      &pht_ctx::sp_grid_cap, cap);
}

extern "C" int pht_ctx_spares_ms(pht_ctx *c, float *vector_ms, float *unit_ms) {
  return clock_read("pht_ctx_spares_ms", c, &pht_ctx::sp_clk, vector_ms, unit_ms);
}

extern "C" int pht_ctx_spares(pht_ctx *c, int ndraws, const double *S, const double *s, int nh, const double *horizons,
                              int batch, long long *words_out, double *scales_out, double *dsum_out, double *vsum_out,
                              double *d2sum_out, long long *cnt_out, double *d_out, double *var_out,
                              int *draw_flags_out) {
  /* the censored units are the forecast's list (read only here) */
  if (censored_units(c, "pht_ctx_spares", PHT_CD_MAXUNITS)) return -1;
  const auto &fc = c->obs.fc;
  if (!horizons_ok("pht_ctx_spares", nh, horizons, 1, PHT_CD_MAXH, pht_sp_horizons_ok)) return -1;
  if (ndraws < 1 || !S || !s || !words_out || !scales_out || !dsum_out || !vsum_out || !d2sum_out || !cnt_out ||
      (d_out && !var_out) || batch < 1 || batch > kLoglikBatch) {
    set_err("pht_ctx_spares: need ndraws >= 1, S, s, words_out, scales_out, dsum_out, vsum_out, d2sum_out, cnt_out, "
            "var_out with d_out and 1 <= batch <= %d",
            kLoglikBatch);
    return -1;
  }
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream.get();
  ctx_drain(c);
  const int n = c->n;
  const long nc = fc.ncens;
  /* under 80 KB of LDS a block: two blocks a CU */
  const int grid_cap = c->sp_grid_cap ? c->sp_grid_cap : 2 * cu_count(c);
  if (grid_cap < 0) return -1;

  /* the draws' meta words (K for the largest age) and Kr; the specification's
   * own flags go into the meta flag word with the evaluator's */
  const int nw = pht_sp_nwords(nh), nvec = spares_vec_doubles(n, nh), ns = 3 * nh + 1, npw = 2 * nh;
  const double hmax = horizons[nh - 1];
  std::vector<int> kr((size_t)ndraws, 0);
  int Krcall = 0;
  const UnifPlan plan(n, ndraws, S, s, batch, draw_flags_out, [&](int d, const double *Sd, const double *sd, double *m) {
    unsigned flag = pht_llu_meta(n, Sd, sd, fc.ymax_c, m);
    if (!flag) {
      flag = pht_sp_flags(n, Sd, sd, m[PHT_LLU_M_MU], hmax);
      if (flag) {
        m[PHT_LLU_M_FLAG] = pht_u2d((uint64_t)flag);
        m[PHT_LLU_M_MU] = m[PHT_LLU_M_ABAR] = m[PHT_LLU_M_K] = 0.0;
      } else {
        kr[(size_t)d] = pht_llu_K(m[PHT_LLU_M_MU], hmax);
        Krcall = std::max(Krcall, kr[(size_t)d]);
      }
    }
    return flag;
  });
  const int Kcall = plan.Kcall, bmax = plan.bmax;
  const long fstride = (long)(Kcall + 1) * n, wstride = (long)PHT_SP_WDOUBLES(nh, Krcall + 1);
  const bool pw = d_out != nullptr;
  const size_t nwords = (size_t)ndraws * nw, nstate = (size_t)nc * ns;
  if (unif_stage(c, plan, S, s)) return -1;
  HIPCHK(ensure(c->d_spF, (size_t)bmax * fstride));
  HIPCHK(ensure(c->d_sph, (size_t)nh));
  HIPCHK(ensure(c->d_spkr, (size_t)ndraws));
  HIPCHK(ensure(c->d_spW, (size_t)bmax * wstride));
  HIPCHK(ensure(c->d_spvec, (size_t)bmax * nvec));
  HIPCHK(ensure(c->d_spwords, nwords));
  HIPCHK(ensure(c->d_spstate, nstate));
  if (pw) HIPCHK(ensure(c->d_sppw, (size_t)nc * bmax * npw));
  HIPCHK(hipMemcpyAsync(c->d_sph.get(), horizons, sizeof(double) * nh, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->d_spkr.get(), kr.data(), sizeof(int) * kr.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(c->d_spwords.get(), 0, sizeof(unsigned long long) * nwords, st));
  HIPCHK(hipMemsetAsync(c->d_spstate.get(), 0, sizeof(double) * nstate, st));
  std::vector<double> hpw, hvec((size_t)bmax * nvec);
  if (pw) hpw.resize((size_t)nc * bmax * npw);
  PhaseClock &clk = c->sp_clk;
  if (clk.begin()) return -1;
  for (int d0 = 0; d0 < ndraws; d0 += batch) {
    const int nb = std::min(batch, ndraws - d0);
    if (clk.mark(0, st)) return -1;
    LlunifTableArgs t;
    if (unif_tables(c, plan, d0, nb, t)) return -1;
    if (cond_forward(c, t, c->d_spF.get(), fstride, Kcall + 1, nb)) return -1;
    SparesVecArgs v{};
    v.n = n;
    v.nd = nb;
    v.nh = nh;
    v.S = t.S;
    v.s = t.s;
    v.meta = t.meta;
    v.h = c->d_sph.get();
    v.kr = c->d_spkr.get() + d0;
    v.W = c->d_spW.get();
    v.wstride = wstride;
    v.rows = Krcall + 1;
    v.vec = c->d_spvec.get();
    HIPCHK(pht_launch_spares_vectors(&v, st));
    if (clk.mark(1, st)) return -1;
    SparesArgs a{};
    a.n = n;
    a.nd = nb;
    a.nh = nh;
    a.Kmax = plan.Kmax(d0, nb);
    a.count = nc;
    a.age = fc.d_age.get();
    a.meta = t.meta;
    a.tab = t.tab;
    a.stride = t.stride;
    a.F = c->d_spF.get();
    a.fstride = fstride;
    a.vec = v.vec;
    a.words = c->d_spwords.get() + (size_t)d0 * nw;
    a.state = c->d_spstate.get();
    a.pw = pw ? c->d_sppw.get() : nullptr;
    HIPCHK(pht_launch_spares(&a, grid_cap, st));
    if (clk.mark(2, st)) return -1;
    HIPCHK(hipMemcpyAsync(hvec.data(), v.vec, sizeof(double) * (size_t)nb * nvec, hipMemcpyDeviceToHost, st));
    if (pw)
      HIPCHK(hipMemcpyAsync(hpw.data(), c->d_sppw.get(), sizeof(double) * (size_t)nc * nb * npw, hipMemcpyDeviceToHost,
                            st));
    HIPCHK(hipStreamSynchronize(st));
    if (clk.add_after_sync()) return -1;
    /* the scales of the batch's usable draws (a flagged draw's vectors were never written) */
    for (int d = 0; d < nb; d++) {
      double *sc = scales_out + (size_t)(d0 + d) * npw;
      const double *src = hvec.data() + (size_t)d * nvec + (size_t)2 * nh * n;
      for (int j = 0; j < npw; j++) sc[j] = plan.flagged(d0 + d) ? 0.0 : src[j];
    }
    if (pw) { /* [unit][draw][D, var] back into the caller's order of the censored observations */
      for (long u = 0; u < nc; u++) {
        const size_t r = (size_t)fc.rank[u];
        for (int d = 0; d < nb; d++) {
          const double *src = hpw.data() + ((size_t)u * nb + d) * npw;
          const size_t cell = ((size_t)(d0 + d) * nc + r) * nh;
          memcpy(d_out + cell, src, sizeof(double) * nh);
          memcpy(var_out + cell, src + nh, sizeof(double) * nh);
        }
      }
    }
  }
  c->last_ms = clk.total();
  std::vector<double> hs(nstate);
  HIPCHK(hipMemcpyAsync(words_out, c->d_spwords.get(), sizeof(long long) * nwords, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hs.data(), c->d_spstate.get(), sizeof(double) * nstate, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  /* every unit of an evaluated draw is good or bad: nunits = ncens - nbad */
  for (int d = 0; d < ndraws; d++) {
    if (plan.flagged(d)) continue;
    long long *w = words_out + (size_t)d * nw;
    w[pht_sp_w_nunits(nh)] = (long long)nc - w[pht_sp_w_nbad(nh)];
  }
  for (long u = 0; u < nc; u++) {
    const size_t r = (size_t)fc.rank[u];
    const double *src = hs.data() + (size_t)u * ns;
    memcpy(dsum_out + r * nh, src, sizeof(double) * nh);
    memcpy(vsum_out + r * nh, src + nh, sizeof(double) * nh);
    memcpy(d2sum_out + r * nh, src + 2 * nh, sizeof(double) * nh);
    cnt_out[r] = (long long)src[3 * nh];
  }
  return 0;
}
