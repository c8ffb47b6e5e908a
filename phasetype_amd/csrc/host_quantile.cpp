/*
 * host_quantile.cpp — quantiles and residual-life quantiles of draws
 * (specification: include/pht_quantile.h; kernel: pht_quantile.hip, the
 * tables by pht_loglik_unif.hip's table kernel).  No reference counterpart.
 * pht_ctx_quantile runs draws x probabilities root searches on the device; it
 * needs no resident observations.  pht_quantile_host is the specification's
 * function for one draw on the host (no device).
 */
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <numeric>

#include "host_internal.h"
#include "pht_loglik_unif_args.h"
#include "pht_quantile.h"
#include "pht_quantile_args.h"

using namespace pht;
using namespace pht::host;

namespace {
constexpr int kQuantMaxP = 1 << 20; /* probabilities of a call */

bool tmax_ok(double tmax) { return tmax > 0.0; /* +inf: as far as the table cap allows */ }
}  // namespace

extern "C" int pht_quantile_host(int n, const double *S, const double *s, int np, const double *probs, double t0,
                                 double tmax, double *t_out, double *lo_out, double *hi_out, int *nev_out,
                                 unsigned *flags_out) {
  if (n < 1 || n > kMaxN || !S || !s || np < 1 || np > kQuantMaxP || !probs || !t_out) {
    set_err("pht_quantile_host: need 1 <= n <= %d, S, s, 1 <= np <= %d, probs and t_out", kMaxN, kQuantMaxP);
    return -1;
  }
  if (!tmax_ok(tmax)) {
    set_err("pht_quantile_host: tmax must be positive (+inf: as far as the table cap allows)");
    return -1;
  }
  std::vector<double> tab(3 * (size_t)(PHT_LLU_MAXK + 1));
  return (int)pht_q_draw(n, S, s, np, probs, t0, tmax, tab.data(), tab.data() + 2 * (PHT_LLU_MAXK + 1), t_out, lo_out,
                         hi_out, nev_out, flags_out);
}

extern "C" int pht_ctx_quantile_ms(pht_ctx *c, float *table_ms, float *search_ms) {
  return clock_read("pht_ctx_quantile_ms", c, &pht_ctx::q_clk, table_ms, search_ms);
}

extern "C" int pht_ctx_quantile(pht_ctx *c, int ndraws, const double *S, const double *s, int np, const double *probs,
                                double t0, double tmax, int batch, double *t_out, double *lo_out, double *hi_out,
                                int *nev_out, unsigned *flags_out, int *draw_flags_out) {
  if (!c) {
    set_err("pht_ctx_quantile: null context");
    return -1;
  }
  if (ndraws < 1 || !S || !s || np < 1 || np > kQuantMaxP || !probs || !t_out || batch < 1 || batch > kLoglikBatch) {
    set_err("pht_ctx_quantile: need ndraws >= 1, S, s, 1 <= np <= %d, probs, t_out and 1 <= batch <= %d", kQuantMaxP,
            kLoglikBatch);
    return -1;
  }
  if (!tmax_ok(tmax)) {
    set_err("pht_ctx_quantile: tmax must be positive (+inf: as far as the table cap allows)");
    return -1;
  }
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream.get();
  ctx_drain(c);
  const int n = c->n;

  /* the probabilities once in ascending order (NaN last; equal ones keep the
   * caller's order): neighbouring lanes then walk neighbouring windows */
  std::vector<int> perm(np);
  std::iota(perm.begin(), perm.end(), 0);
  std::stable_sort(perm.begin(), perm.end(), [&](int x, int y) {
    const double px = probs[x], py = probs[y];
    if (std::isnan(px) || std::isnan(py)) return !std::isnan(px) && std::isnan(py);
    return px < py;
  });
  std::vector<double> psort(np);
  for (int i = 0; i < np; i++) psort[i] = probs[perm[i]];

  std::vector<double> thi(ndraws);
  const UnifPlan plan(n, ndraws, S, s, batch, draw_flags_out, [&](int d, const double *Sd, const double *sd, double *m) {
    return pht_q_meta(n, Sd, sd, tmax, m, &thi[d]);
  });
  const size_t cells = (size_t)plan.bmax * np;
  if (unif_stage(c, plan, S, s)) return -1;
  HIPCHK(ensure(c->d_qin, (size_t)np + ndraws));
  HIPCHK(ensure(c->d_qout, 3 * cells));
  HIPCHK(ensure(c->d_qouti, 2 * cells));
  double *dprobs = c->d_qin.get(), *dthi = dprobs + np;
  HIPCHK(hipMemcpyAsync(dprobs, psort.data(), sizeof(double) * np, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dthi, thi.data(), sizeof(double) * ndraws, hipMemcpyHostToDevice, st));
  std::vector<double> hd(3 * cells);
  std::vector<int> hi(2 * cells);
  PhaseClock &clk = c->q_clk;
  if (clk.begin()) return -1;
  for (int d0 = 0; d0 < ndraws; d0 += batch) {
    const int nb = std::min(batch, ndraws - d0), Kmax = plan.Kmax(d0, nb);
    const size_t nc = (size_t)nb * np;
    if (clk.mark(0, st)) return -1;
    LlunifTableArgs t;
    if (unif_tables(c, plan, d0, nb, t)) return -1;
    if (clk.mark(1, st)) return -1;
    QuantileArgs a{};
    int pool = 1;
    a.nd = nb;
    a.np = np;
    a.Kmax = Kmax;
    a.dpb = pht_quantile_pack(nb, np, Kmax, &pool);
    a.lp = std::min(np, kQuantBlock);
    a.meta = t.meta;
    a.thi = dthi + d0;
    a.tab = t.tab;
    a.stride = t.stride;
    a.probs = dprobs;
    a.t0 = t0;
    a.t = c->d_qout.get();
    a.lo = a.t + nc;
    a.hi = a.lo + nc;
    a.nev = c->d_qouti.get();
    a.flags = reinterpret_cast<unsigned *>(a.nev + nc);
    HIPCHK(pht_launch_quantile(&a, st));
    if (clk.mark(2, st)) return -1;
    HIPCHK(hipMemcpyAsync(hd.data(), c->d_qout.get(), sizeof(double) * 3 * nc, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hi.data(), c->d_qouti.get(), sizeof(int) * 2 * nc, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (clk.add_after_sync()) return -1;
    /* back into the caller's order */
    for (int d = 0; d < nb; d++) {
      const size_t src = (size_t)d * np, dst = (size_t)(d0 + d) * np;
      for (int i = 0; i < np; i++) {
        const size_t o = dst + perm[i];
        t_out[o] = hd[src + i];
        if (lo_out) lo_out[o] = hd[nc + src + i];
        if (hi_out) hi_out[o] = hd[2 * nc + src + i];
        if (nev_out) nev_out[o] = hi[src + i];
        if (flags_out) flags_out[o] = (unsigned)hi[nc + src + i];
      }
    }
  }
  c->last_ms = clk.total();
  return 0;
}
