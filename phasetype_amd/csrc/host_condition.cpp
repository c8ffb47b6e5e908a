/*
 * host_condition.cpp — fleet condition: the posterior law of the phase of
 * every censored unit of the context for every draw, its mean residual life
 * and its expected failures with replacement (specification:
 * include/pht_condition.h; kernels: pht_condition.hip, the (ax, ac) tables by
 * pht_loglik_unif.hip's table kernel).  No reference counterpart.
 * pht_ctx_condition runs draws x censored units windows on the device over the
 * context's resident observations; the draws' vectors m, r_h and scales are
 * computed here from the same header (pht_cd_vectors).  pht_condition_host is
 * the specification's function for one draw on the host (no device).
 */
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include "host_internal.h"
#include "pht_condition.h"
#include "pht_condition_args.h"
#include "pht_loglik_unif_args.h"

using namespace pht;
using namespace pht::host;

extern "C" int pht_condition_host(int n, const double *S, const double *s, long ncens, const double *ages, int nh,
                                  const double *horizons, double ymax_c, long long *words_out, double *scales_out,
                                  double *phisum, double *mrlsum, double *dsum, long long *cnt, double *phi_out,
                                  double *mrl_out, double *d_out) {
  if (n < 1 || n > kMaxN || !S || !s || !ages || !words_out || !scales_out) {
    set_err("pht_condition_host: need 1 <= n <= %d, S, s, ages, words_out and scales_out", kMaxN);
    return -1;
  }
  const char *who = "pht_condition_host";
  double ymax = 0.0;
  if (!units_ok(who, ncens, PHT_CD_MAXUNITS) || !horizons_ok(who, nh, horizons, 0, PHT_CD_MAXH, pht_cd_horizons_ok) ||
      !ymax_c_ok(who, ncens, ages, ymax_c, &ymax))
    return -1;
  std::vector<double> work(PHT_CD_WORK(n, nh));
  return (int)pht_cd_draw(n, S, s, ncens, ages, ymax, nh, horizons, work.data(), words_out, scales_out, phisum, mrlsum,
                          dsum, cnt, phi_out, mrl_out, d_out);
}

extern "C" int pht_ctx_condition_grid_cap(pht_ctx *c, int cap) {
  return grid_cap_set("pht_ctx_condition_grid_cap", "need a context and cap >= 0 (0: the default)", c,
                      &pht_ctx::cd_grid_cap, cap);
}

extern "C" int pht_ctx_condition_ms(pht_ctx *c, float *table_ms, float *unit_ms) {
  return clock_read("pht_ctx_condition_ms", c, &pht_ctx::cd_clk, table_ms, unit_ms);
}

extern "C" int pht_ctx_condition(pht_ctx *c, int ndraws, const double *S, const double *s, int nh,
                                 const double *horizons, int batch, long long *words_out, double *scales_out,
                                 double *phisum_out, double *mrlsum_out, double *dsum_out, long long *cnt_out,
                                 double *phi_out, double *mrl_out, double *d_out, int *draw_flags_out) {
  /* the censored units are the forecast's list (read only here) */
  if (censored_units(c, "pht_ctx_condition", PHT_CD_MAXUNITS)) return -1;
  const auto &fc = c->obs.fc;
  if (!horizons_ok("pht_ctx_condition", nh, horizons, 0, PHT_CD_MAXH, pht_cd_horizons_ok)) return -1;
  if (ndraws < 1 || !S || !s || !words_out || !scales_out || !phisum_out || !mrlsum_out || (nh > 0 && !dsum_out) ||
      !cnt_out || batch < 1 || batch > kLoglikBatch) {
    set_err("pht_ctx_condition: need ndraws >= 1, S, s, words_out, scales_out, phisum_out, mrlsum_out, dsum_out, "
            "cnt_out and 1 <= batch <= %d",
            kLoglikBatch);
    return -1;
  }
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream.get();
  ctx_drain(c);
  const int n = c->n;
  const long nc = fc.ncens;
  /* under 80 KB of LDS a block at n <= 20: two blocks a CU */
  const int grid_cap = c->cd_grid_cap ? c->cd_grid_cap : 2 * cu_count(c);
  if (grid_cap < 0) return -1;

  /* the draws' meta words (K for the largest age), vectors and scales; the
   * specification's own flags go into the meta flag word with the evaluator's */
  const int nw = pht_cd_nwords(n, nh), nvec = cond_vec_doubles(n, nh), ns = n + 1 + nh;
  std::vector<double> vec((size_t)ndraws * nvec, 0.0), T((size_t)std::max(nh, 1) * (PHT_LLU_MAXK + 1));
  const UnifPlan plan(n, ndraws, S, s, batch, draw_flags_out, [&](int d, const double *Sd, const double *sd, double *m) {
    double *v = vec.data() + (size_t)d * nvec;
    unsigned flag = pht_llu_meta(n, Sd, sd, fc.ymax_c, m);
    if (!flag) {
      flag = pht_cd_vectors(n, Sd, sd, m[PHT_LLU_M_MU], nh, horizons, T.data(), v, v + n, v + n + nh * n);
      if (flag) {
        m[PHT_LLU_M_FLAG] = pht_u2d((uint64_t)flag);
        m[PHT_LLU_M_MU] = m[PHT_LLU_M_ABAR] = m[PHT_LLU_M_K] = 0.0;
      }
    }
    for (int j = 0; j <= nh; j++) scales_out[(size_t)d * (1 + nh) + j] = flag ? 0.0 : v[n + nh * n + j];
    return flag;
  });
  const int Kcall = plan.Kcall, bmax = plan.bmax;
  const long fstride = (long)(Kcall + 1) * n;
  const bool pw = phi_out != nullptr;
  const size_t nwords = (size_t)ndraws * nw, nstate = (size_t)nc * (ns + 1);
  if (unif_stage(c, plan, S, s)) return -1;
  HIPCHK(ensure(c->d_cdF, (size_t)bmax * fstride));
  HIPCHK(ensure(c->d_cdvec, vec.size()));
  HIPCHK(ensure(c->d_cdwords, nwords));
  HIPCHK(ensure(c->d_cdstate, nstate));
  if (pw) HIPCHK(ensure(c->d_cdpw, (size_t)nc * bmax * ns));
  HIPCHK(hipMemcpyAsync(c->d_cdvec.get(), vec.data(), sizeof(double) * vec.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(c->d_cdwords.get(), 0, sizeof(unsigned long long) * nwords, st));
  HIPCHK(hipMemsetAsync(c->d_cdstate.get(), 0, sizeof(double) * nstate, st));
  std::vector<double> hpw;
  if (pw) hpw.resize((size_t)nc * bmax * ns);
  PhaseClock &clk = c->cd_clk;
  if (clk.begin()) return -1;
  for (int d0 = 0; d0 < ndraws; d0 += batch) {
    const int nb = std::min(batch, ndraws - d0);
    if (clk.mark(0, st)) return -1;
    LlunifTableArgs t;
    if (unif_tables(c, plan, d0, nb, t)) return -1;
    if (cond_forward(c, t, c->d_cdF.get(), fstride, Kcall + 1, nb)) return -1;
    if (clk.mark(1, st)) return -1;
    CondArgs a{};
    a.n = n;
    a.nd = nb;
    a.nh = nh;
    a.Kmax = plan.Kmax(d0, nb);
    a.count = nc;
    a.age = fc.d_age.get();
    a.meta = t.meta;
    a.tab = t.tab;
    a.stride = t.stride;
    a.F = c->d_cdF.get();
    a.fstride = fstride;
    a.vec = c->d_cdvec.get() + (size_t)d0 * nvec;
    a.words = c->d_cdwords.get() + (size_t)d0 * nw;
    a.state = c->d_cdstate.get();
    a.pw = pw ? c->d_cdpw.get() : nullptr;
    HIPCHK(pht_launch_cond(&a, grid_cap, st));
    if (clk.mark(2, st)) return -1;
    if (pw)
      HIPCHK(hipMemcpyAsync(hpw.data(), c->d_cdpw.get(), sizeof(double) * (size_t)nc * nb * ns, hipMemcpyDeviceToHost,
                            st));
    HIPCHK(hipStreamSynchronize(st));
    if (clk.add_after_sync()) return -1;
    if (pw) { /* [unit][draw][phi, MRL, D] back into the caller's order of the censored observations */
      for (long u = 0; u < nc; u++) {
        const size_t r = (size_t)fc.rank[u];
        for (int d = 0; d < nb; d++) {
          const double *src = hpw.data() + ((size_t)u * nb + d) * ns;
          const size_t cell = (size_t)(d0 + d) * nc + r;
          memcpy(phi_out + cell * n, src, sizeof(double) * n);
          if (mrl_out) mrl_out[cell] = src[n];
          if (d_out && nh) memcpy(d_out + cell * nh, src + n + 1, sizeof(double) * nh);
        }
      }
    }
  }
  c->last_ms = clk.total();
  std::vector<double> hs(nstate);
  HIPCHK(hipMemcpyAsync(words_out, c->d_cdwords.get(), sizeof(long long) * nwords, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hs.data(), c->d_cdstate.get(), sizeof(double) * nstate, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  /* every unit of an evaluated draw is good or bad: nunits = ncens - nbad */
  for (int d = 0; d < ndraws; d++) {
    if (plan.flagged(d)) continue;
    long long *w = words_out + (size_t)d * nw;
    w[pht_cd_w_nunits(n, nh)] = (long long)nc - w[pht_cd_w_nbad(n, nh)];
  }
  for (long u = 0; u < nc; u++) {
    const size_t r = (size_t)fc.rank[u];
    const double *src = hs.data() + (size_t)u * (ns + 1);
    memcpy(phisum_out + r * n, src, sizeof(double) * n);
    mrlsum_out[r] = src[n];
    if (nh) memcpy(dsum_out + r * nh, src + n + 1, sizeof(double) * nh);
    cnt_out[r] = (long long)src[ns];
  }
  return 0;
}
