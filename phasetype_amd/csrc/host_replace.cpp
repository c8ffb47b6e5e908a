/*
 * host_replace.cpp — age-replacement policies of draws (specification:
 * include/pht_replace.h; kernels: pht_replace.hip, the tables by
 * pht_loglik_unif.hip's table kernel).  No reference counterpart.
 * pht_ctx_replace runs the curve (draws x ages) and the policies (draws x cost
 * pairs) on the device; it needs no resident observations.  pht_replace_host
 * is the specification's function for one draw on the host (no device).
 */
#include <math.h>
#include <string.h>

#include <algorithm>

#include "host_internal.h"
#include "pht_loglik_unif_args.h"
#include "pht_replace.h"
#include "pht_replace_args.h"

using namespace pht;
using namespace pht::host;

namespace {
bool shape_ok(const char *who, int G, const double *ages, int P, const double *cp, const double *cf) {
  if (G < 1 || G > PHT_RP_MAXG || !ages) {
    set_err("%s: need 1 <= G <= %d ages", who, PHT_RP_MAXG);
    return false;
  }
  if (!pht_rp_ages_ok(G, ages)) {
    set_err("%s: the ages must be finite, positive and strictly increasing", who);
    return false;
  }
  if (P < 1 || P > PHT_RP_MAXP || !cp || !cf) {
    set_err("%s: need 1 <= P <= %d cost pairs (cp, cf)", who, PHT_RP_MAXP);
    return false;
  }
  return true;
}
}  // namespace

extern "C" int pht_replace_host(int n, const double *S, const double *s, int G, const double *ages, int P,
                                const double *cp, const double *cf, double *t_out, double *g_out, double *lo_out,
                                double *hi_out, int *j_out, int *nev_out, unsigned *flags_out, double *m_out,
                                double *lS_out, double *lf_out, double *M_out, unsigned *aflags_out) {
  if (n < 1 || n > kMaxN || !S || !s) {
    set_err("pht_replace_host: need 1 <= n <= %d, S and s", kMaxN);
    return -1;
  }
  if (!shape_ok("pht_replace_host", G, ages, P, cp, cf)) return -1;
  if (!t_out || !g_out || !lo_out || !hi_out || !j_out || !nev_out || !flags_out || !m_out) {
    set_err("pht_replace_host: need every policy output and m_out");
    return -1;
  }
  std::vector<double> work(PHT_RP_WORK(G));
  std::vector<unsigned> af((size_t)G);
  const unsigned flag = pht_rp_draw(n, S, s, G, ages, P, cp, cf, work.data(), af.data(), lS_out, lf_out, M_out, m_out,
                                    t_out, g_out, lo_out, hi_out, j_out, nev_out, flags_out);
  if (aflags_out) memcpy(aflags_out, af.data(), sizeof(unsigned) * (size_t)G);
  return (int)flag;
}

extern "C" int pht_ctx_replace_ms(pht_ctx *c, float *curve_ms, float *policy_ms) {
  return clock_read("pht_ctx_replace_ms", c, &pht_ctx::rp_clk, curve_ms, policy_ms);
}

extern "C" int pht_ctx_replace(pht_ctx *c, int ndraws, const double *S, const double *s, int G, const double *ages,
                               int P, const double *cp, const double *cf, int batch, double *t_out, double *g_out,
                               double *lo_out, double *hi_out, int *j_out, int *nev_out, unsigned *flags_out,
                               double *m_out, int *draw_flags_out, double *lS_out, double *lf_out, double *M_out,
                               unsigned *aflags_out) {
  if (!c) {
    set_err("pht_ctx_replace: null context");
    return -1;
  }
  if (c->n > kMaxN) {
    set_err("pht_ctx_replace: need n <= %d", kMaxN);
    return -1;
  }
  if (ndraws < 1 || !S || !s || batch < 1 || batch > kLoglikBatch) {
    set_err("pht_ctx_replace: need ndraws >= 1, S, s and 1 <= batch <= %d", kLoglikBatch);
    return -1;
  }
  if (!shape_ok("pht_ctx_replace", G, ages, P, cp, cf)) return -1;
  if (!t_out || !g_out) {
    set_err("pht_ctx_replace: need t_out and g_out");
    return -1;
  }
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream.get();
  ctx_drain(c);
  const int n = c->n;

  std::vector<double> thi(ndraws), mean(ndraws);
  const UnifPlan plan(n, ndraws, S, s, batch, draw_flags_out, [&](int d, const double *Sd, const double *sd, double *m) {
    return pht_rp_meta(n, Sd, sd, ages[G - 1], m, &thi[d], &mean[d]);
  });
  if (m_out) std::copy(mean.begin(), mean.end(), m_out);
  const size_t bmax = (size_t)plan.bmax, ccstride = (size_t)plan.Kcall + 1;
  const size_t ncur = bmax * G, npol = bmax * P;
  if (unif_stage(c, plan, S, s)) return -1;
  HIPCHK(ensure(c->d_rpin, (size_t)G + 2 * (size_t)P + 2 * (size_t)ndraws));
  HIPCHK(ensure(c->d_rpcc, bmax * ccstride));
  HIPCHK(ensure(c->d_rpout, 3 * ncur + 4 * npol));
  HIPCHK(ensure(c->d_rpouti, ncur + 3 * npol));
  double *dages = c->d_rpin.get(), *dcp = dages + G, *dcf = dcp + P, *dthi = dcf + P, *dmean = dthi + ndraws;
  HIPCHK(hipMemcpyAsync(dages, ages, sizeof(double) * G, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dcp, cp, sizeof(double) * P, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dcf, cf, sizeof(double) * P, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dthi, thi.data(), sizeof(double) * ndraws, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dmean, mean.data(), sizeof(double) * ndraws, hipMemcpyHostToDevice, st));
  std::vector<double> hd(3 * ncur + 4 * npol);
  std::vector<int> hi(ncur + 3 * npol);
  PhaseClock &clk = c->rp_clk;
  if (clk.begin()) return -1;
  for (int d0 = 0; d0 < ndraws; d0 += batch) {
    const int nb = std::min(batch, ndraws - d0), Kmax = plan.Kmax(d0, nb);
    const size_t nc = (size_t)nb * G, np = (size_t)nb * P;
    if (clk.mark(0, st)) return -1;
    LlunifTableArgs t;
    if (unif_tables(c, plan, d0, nb, t)) return -1;
    ReplaceCurveArgs a{};
    a.nd = nb;
    a.G = G;
    a.Kmax = Kmax;
    a.dpb = pht_replace_pack(nb, G, Kmax);
    a.lp = std::min(G, kRpBlock);
    a.meta = t.meta;
    a.thi = dthi + d0;
    a.tab = t.tab;
    a.stride = t.stride;
    a.ages = dages;
    a.cc = c->d_rpcc.get();
    a.ccstride = (int)ccstride;
    a.lS = c->d_rpout.get();
    a.lf = a.lS + nc;
    a.M = a.lf + nc;
    a.aflags = reinterpret_cast<unsigned *>(c->d_rpouti.get());
    HIPCHK(pht_launch_replace_curve(&a, st));
    if (clk.mark(1, st)) return -1;
    ReplacePolicyArgs b{};
    b.nd = nb;
    b.G = G;
    b.P = P;
    b.Kmax = Kmax;
    b.meta = t.meta;
    b.mean = dmean + d0;
    b.tab = t.tab;
    b.stride = t.stride;
    b.cc = a.cc;
    b.ccstride = a.ccstride;
    b.ages = dages;
    b.lS = a.lS;
    b.lf = a.lf;
    b.M = a.M;
    b.aflags = a.aflags;
    b.cp = dcp;
    b.cf = dcf;
    b.t = a.M + nc;
    b.g = b.t + np;
    b.lo = b.g + np;
    b.hi = b.lo + np;
    b.j = c->d_rpouti.get() + nc;
    b.nev = b.j + np;
    b.flags = reinterpret_cast<unsigned *>(b.nev + np);
    HIPCHK(pht_launch_replace_policy(&b, st));
    if (clk.mark(2, st)) return -1;
    HIPCHK(hipMemcpyAsync(hd.data(), c->d_rpout.get(), sizeof(double) * (3 * nc + 4 * np), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hi.data(), c->d_rpouti.get(), sizeof(int) * (nc + 3 * np), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (clk.add_after_sync()) return -1;
    const size_t cd = (size_t)d0 * G, pd = (size_t)d0 * P;
    if (lS_out) std::copy(hd.begin(), hd.begin() + nc, lS_out + cd);
    if (lf_out) std::copy(hd.begin() + nc, hd.begin() + 2 * nc, lf_out + cd);
    if (M_out) std::copy(hd.begin() + 2 * nc, hd.begin() + 3 * nc, M_out + cd);
    if (aflags_out)
      for (size_t i = 0; i < nc; i++) aflags_out[cd + i] = (unsigned)hi[i];
    const double *hp = hd.data() + 3 * nc;
    std::copy(hp, hp + np, t_out + pd);
    std::copy(hp + np, hp + 2 * np, g_out + pd);
    if (lo_out) std::copy(hp + 2 * np, hp + 3 * np, lo_out + pd);
    if (hi_out) std::copy(hp + 3 * np, hp + 4 * np, hi_out + pd);
    const int *ip = hi.data() + nc;
    if (j_out) std::copy(ip, ip + np, j_out + pd);
    if (nev_out) std::copy(ip + np, ip + 2 * np, nev_out + pd);
    if (flags_out)
      for (size_t i = 0; i < np; i++) flags_out[pd + i] = (unsigned)ip[2 * np + i];
  }
  c->last_ms = clk.total();
  return 0;
}
