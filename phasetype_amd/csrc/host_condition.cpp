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

namespace {

/* what both entry points refuse about the horizons */
bool horizons_ok(const char *who, int nh, const double *h) {
  if (nh < 0 || nh > PHT_CD_MAXH || (nh > 0 && !h)) {
    set_err("%s: need 0 <= nh <= %d horizons", who, PHT_CD_MAXH);
    return false;
  }
  if (!pht_cd_horizons_ok(nh, h)) {
    set_err("%s: every horizon must be finite, >= 0 and larger than the one before", who);
    return false;
  }
  return true;
}

}  // namespace

extern "C" int pht_condition_host(int n, const double *S, const double *s, long ncens, const double *ages, int nh,
                                  const double *horizons, double ymax_c, long long *words_out, double *scales_out,
                                  double *phisum, double *mrlsum, double *dsum, long long *cnt, double *phi_out,
                                  double *mrl_out, double *d_out) {
  if (n < 1 || n > kMaxN || !S || !s || !ages || !words_out || !scales_out) {
    set_err("pht_condition_host: need 1 <= n <= %d, S, s, ages, words_out and scales_out", kMaxN);
    return -1;
  }
  if (ncens < 1) {
    set_err("pht_condition_host: no censored unit (ncens >= 1)");
    return -1;
  }
  if (ncens > PHT_CD_MAXUNITS) {
    set_err("pht_condition_host: %ld censored units, at most %ld (the int64 sums)", ncens, (long)PHT_CD_MAXUNITS);
    return -1;
  }
  if (!horizons_ok("pht_condition_host", nh, horizons)) return -1;
  double amax = 0.0;
  for (long i = 0; i < ncens; i++) amax = (ages[i] > amax) ? ages[i] : amax;
  if (ymax_c != 0.0 && !(ymax_c >= amax && ymax_c < INFINITY)) {
    set_err("pht_condition_host: ymax_c must be 0 (the largest age) or finite and at least the largest age");
    return -1;
  }
  std::vector<double> work(PHT_CD_WORK(n, nh));
  return (int)pht_cd_draw(n, S, s, ncens, ages, ymax_c != 0.0 ? ymax_c : amax, nh, horizons, work.data(), words_out,
                          scales_out, phisum, mrlsum, dsum, cnt, phi_out, mrl_out, d_out);
}

extern "C" int pht_ctx_condition_grid_cap(pht_ctx *c, int cap) {
  if (!c || cap < 0) {
    set_err("pht_ctx_condition_grid_cap: need a context and cap >= 0 (0: the default)");
    return -1;
  }
  c->cd_grid_cap = cap;
  return 0;
}

extern "C" int pht_ctx_condition_ms(pht_ctx *c, float *table_ms, float *unit_ms) {
  if (!c) {
    set_err("pht_ctx_condition_ms: null context");
    return -1;
  }
  if (table_ms) *table_ms = c->cd_ms[0];
  if (unit_ms) *unit_ms = c->cd_ms[1];
  return 0;
}

extern "C" int pht_ctx_condition(pht_ctx *c, int ndraws, const double *S, const double *s, int nh,
                                 const double *horizons, int batch, long long *words_out, double *scales_out,
                                 double *phisum_out, double *mrlsum_out, double *dsum_out, long long *cnt_out,
                                 double *phi_out, double *mrl_out, double *d_out, int *draw_flags_out) {
  if (!c) {
    set_err("pht_ctx_condition: null context");
    return -1;
  }
  /* the censored units are the forecast's list (read only here) */
  if (pht_ctx_forecast_units(c, nullptr) < 0) return -1;
  const auto &fc = c->obs.fc;
  if (fc.ncens < 1) {
    set_err("pht_ctx_condition: no censored observation on this context (pht_ctx_set_obs)");
    return -1;
  }
  if (fc.ncens > PHT_CD_MAXUNITS) {
    set_err("pht_ctx_condition: %ld censored units on this context, at most %ld (the int64 sums): shard them",
            fc.ncens, (long)PHT_CD_MAXUNITS);
    return -1;
  }
  if (!horizons_ok("pht_ctx_condition", nh, horizons)) return -1;
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
  for (auto &e : c->cd_ev)
    if (!e) HIPCHK(e.create());
  int grid_cap = c->cd_grid_cap;
  if (!grid_cap) { /* under 80 KB of LDS a block at n <= 20: two blocks a CU */
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    grid_cap = std::max(1, cus) * 2;
  }

  /* the draws' meta words (K for the largest age), vectors and scales; the
   * specification's own flags go into the meta flag word with the evaluator's */
  const int nw = pht_cd_nwords(n, nh), nvec = cond_vec_doubles(n, nh), ns = n + 1 + nh;
  std::vector<double> meta((size_t)ndraws * PHT_LLU_META), vec((size_t)ndraws * nvec, 0.0);
  std::vector<double> T((size_t)std::max(nh, 1) * (PHT_LLU_MAXK + 1));
  int Kcall = 0;
  for (int d = 0; d < ndraws; d++) {
    double *m = meta.data() + (size_t)d * PHT_LLU_META, *v = vec.data() + (size_t)d * nvec;
    const double *Sd = S + (size_t)d * n * n, *sd = s + (size_t)d * n;
    unsigned flag = pht_llu_meta(n, Sd, sd, fc.ymax_c, m);
    if (!flag) {
      flag = pht_cd_vectors(n, Sd, sd, m[PHT_LLU_M_MU], nh, horizons, T.data(), v, v + n, v + n + nh * n);
      if (flag) {
        m[PHT_LLU_M_FLAG] = pht_u2d((uint64_t)flag);
        m[PHT_LLU_M_MU] = m[PHT_LLU_M_ABAR] = m[PHT_LLU_M_K] = 0.0;
      }
    }
    for (int j = 0; j <= nh; j++) scales_out[(size_t)d * (1 + nh) + j] = flag ? 0.0 : v[n + nh * n + j];
    if (draw_flags_out) draw_flags_out[d] = (int)flag;
    Kcall = std::max(Kcall, (int)m[PHT_LLU_M_K]);
  }
  const int stride = 2 * (Kcall + 1);
  const long fstride = (long)(Kcall + 1) * n;
  const int bmax = std::min(batch, ndraws);
  const bool pw = phi_out != nullptr;
  const size_t nS = (size_t)ndraws * n * n, nsv = (size_t)ndraws * n, nwords = (size_t)ndraws * nw;
  const size_t nstate = (size_t)nc * (ns + 1);
  HIPCHK(ensure(c->d_lluin, c->lluin_cap, nS + nsv + meta.size()));
  HIPCHK(ensure(c->d_llutab, c->llutab_cap, (size_t)bmax * stride));
  HIPCHK(ensure(c->d_cdF, c->cdF_cap, (size_t)bmax * fstride));
  HIPCHK(ensure(c->d_cdvec, c->cdvec_cap, vec.size()));
  HIPCHK(ensure(c->d_cdwords, c->cdwords_cap, nwords));
  HIPCHK(ensure(c->d_cdstate, c->cdstate_cap, nstate));
  if (pw) HIPCHK(ensure(c->d_cdpw, c->cdpw_cap, (size_t)nc * bmax * ns));
  double *dS = c->d_lluin.get(), *ds = dS + nS, *dmeta = ds + nsv;
  HIPCHK(hipMemcpyAsync(dS, S, sizeof(double) * nS, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(ds, s, sizeof(double) * nsv, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dmeta, meta.data(), sizeof(double) * meta.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->d_cdvec.get(), vec.data(), sizeof(double) * vec.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(c->d_cdwords.get(), 0, sizeof(unsigned long long) * nwords, st));
  HIPCHK(hipMemsetAsync(c->d_cdstate.get(), 0, sizeof(double) * nstate, st));
  std::vector<double> hpw;
  if (pw) hpw.resize((size_t)nc * bmax * ns);
  c->cd_ms[0] = c->cd_ms[1] = 0.f;
  for (int d0 = 0; d0 < ndraws; d0 += batch) {
    const int nb = std::min(batch, ndraws - d0);
    int Kmax = 0;
    for (int d = d0; d < d0 + nb; d++) Kmax = std::max(Kmax, (int)meta[(size_t)d * PHT_LLU_META + PHT_LLU_M_K]);
    HIPCHK(hipEventRecord(c->cd_ev[0].get(), st));
    LlunifTableArgs t{};
    t.n = n;
    t.nd = nb;
    t.S = dS + (size_t)d0 * n * n;
    t.s = ds + (size_t)d0 * n;
    t.meta = dmeta + (size_t)d0 * PHT_LLU_META;
    t.tab = c->d_llutab.get();
    t.stride = stride;
    HIPCHK(pht_launch_llunif_table(&t, st));
    CondTableArgs f{};
    f.n = n;
    f.nd = nb;
    f.S = t.S;
    f.meta = t.meta;
    f.F = c->d_cdF.get();
    f.fstride = fstride;
    f.rows = Kcall + 1;
    HIPCHK(pht_launch_cond_forward(&f, st));
    HIPCHK(hipEventRecord(c->cd_ev[1].get(), st));
    CondArgs a{};
    a.n = n;
    a.nd = nb;
    a.nh = nh;
    a.Kmax = Kmax;
    a.count = nc;
    a.age = fc.d_age.get();
    a.meta = t.meta;
    a.tab = t.tab;
    a.stride = stride;
    a.F = f.F;
    a.fstride = fstride;
    a.vec = c->d_cdvec.get() + (size_t)d0 * nvec;
    a.words = c->d_cdwords.get() + (size_t)d0 * nw;
    a.state = c->d_cdstate.get();
    a.pw = pw ? c->d_cdpw.get() : nullptr;
    HIPCHK(pht_launch_cond(&a, grid_cap, st));
    HIPCHK(hipEventRecord(c->cd_ev[2].get(), st));
    if (pw)
      HIPCHK(hipMemcpyAsync(hpw.data(), c->d_cdpw.get(), sizeof(double) * (size_t)nc * nb * ns, hipMemcpyDeviceToHost,
                            st));
    HIPCHK(hipStreamSynchronize(st));
    float ms0 = 0.f, ms1 = 0.f;
    HIPCHK(hipEventElapsedTime(&ms0, c->cd_ev[0].get(), c->cd_ev[1].get()));
    HIPCHK(hipEventElapsedTime(&ms1, c->cd_ev[1].get(), c->cd_ev[2].get()));
    c->cd_ms[0] += ms0;
    c->cd_ms[1] += ms1;
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
  c->last_ms = c->cd_ms[0] + c->cd_ms[1];
  std::vector<double> hs(nstate);
  HIPCHK(hipMemcpyAsync(words_out, c->d_cdwords.get(), sizeof(long long) * nwords, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hs.data(), c->d_cdstate.get(), sizeof(double) * nstate, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  /* every unit of an evaluated draw is good or bad: nunits = ncens - nbad */
  for (int d = 0; d < ndraws; d++) {
    if (pht_d2u(meta[(size_t)d * PHT_LLU_META + PHT_LLU_M_FLAG]) != 0) continue;
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
