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
  if (!c) {
    set_err("pht_ctx_quantile_ms: null context");
    return -1;
  }
  if (table_ms) *table_ms = c->q_ms[0];
  if (search_ms) *search_ms = c->q_ms[1];
  return 0;
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
  for (auto &e : c->q_ev)
    if (!e) HIPCHK(e.create());

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

  std::vector<double> meta((size_t)ndraws * PHT_LLU_META), thi(ndraws);
  int Kcall = 0;
  for (int d = 0; d < ndraws; d++) {
    double *m = meta.data() + (size_t)d * PHT_LLU_META;
    const unsigned flag = pht_q_meta(n, S + (size_t)d * n * n, s + (size_t)d * n, tmax, m, &thi[d]);
    if (draw_flags_out) draw_flags_out[d] = (int)flag;
    Kcall = std::max(Kcall, (int)m[PHT_LLU_M_K]);
  }
  const int stride = 2 * (Kcall + 1);
  const int bmax = std::min(batch, ndraws);
  const size_t nS = (size_t)ndraws * n * n, ns = (size_t)ndraws * n, cells = (size_t)bmax * np;
  HIPCHK(ensure(c->d_lluin, c->lluin_cap, nS + ns + meta.size()));
  HIPCHK(ensure(c->d_llutab, c->llutab_cap, (size_t)bmax * stride));
  HIPCHK(ensure(c->d_qin, c->qin_cap, (size_t)np + ndraws));
  HIPCHK(ensure(c->d_qout, c->qout_cap, 3 * cells));
  HIPCHK(ensure(c->d_qouti, c->qouti_cap, 2 * cells));
  double *dS = c->d_lluin.get(), *ds = dS + nS, *dmeta = ds + ns;
  double *dprobs = c->d_qin.get(), *dthi = dprobs + np;
  HIPCHK(hipMemcpyAsync(dS, S, sizeof(double) * nS, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(ds, s, sizeof(double) * ns, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dmeta, meta.data(), sizeof(double) * meta.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dprobs, psort.data(), sizeof(double) * np, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dthi, thi.data(), sizeof(double) * ndraws, hipMemcpyHostToDevice, st));
  std::vector<double> hd(3 * cells);
  std::vector<int> hi(2 * cells);
  c->q_ms[0] = c->q_ms[1] = 0.f;
  for (int d0 = 0; d0 < ndraws; d0 += batch) {
    const int nb = std::min(batch, ndraws - d0);
    int Kmax = 0;
    for (int d = d0; d < d0 + nb; d++) Kmax = std::max(Kmax, (int)meta[(size_t)d * PHT_LLU_META + PHT_LLU_M_K]);
    const size_t nc = (size_t)nb * np;
    HIPCHK(hipEventRecord(c->q_ev[0].get(), st));
    LlunifTableArgs t{};
    t.n = n;
    t.nd = nb;
    t.S = dS + (size_t)d0 * n * n;
    t.s = ds + (size_t)d0 * n;
    t.meta = dmeta + (size_t)d0 * PHT_LLU_META;
    t.tab = c->d_llutab.get();
    t.stride = stride;
    HIPCHK(pht_launch_llunif_table(&t, st));
    HIPCHK(hipEventRecord(c->q_ev[1].get(), st));
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
    a.stride = stride;
    a.probs = dprobs;
    a.t0 = t0;
    a.t = c->d_qout.get();
    a.lo = a.t + nc;
    a.hi = a.lo + nc;
    a.nev = c->d_qouti.get();
    a.flags = reinterpret_cast<unsigned *>(a.nev + nc);
    HIPCHK(pht_launch_quantile(&a, st));
    HIPCHK(hipEventRecord(c->q_ev[2].get(), st));
    HIPCHK(hipMemcpyAsync(hd.data(), c->d_qout.get(), sizeof(double) * 3 * nc, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hi.data(), c->d_qouti.get(), sizeof(int) * 2 * nc, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms0 = 0.f, ms1 = 0.f;
    HIPCHK(hipEventElapsedTime(&ms0, c->q_ev[0].get(), c->q_ev[1].get()));
    HIPCHK(hipEventElapsedTime(&ms1, c->q_ev[1].get(), c->q_ev[2].get()));
    c->q_ms[0] += ms0;
    c->q_ms[1] += ms1;
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
  c->last_ms = c->q_ms[0] + c->q_ms[1];
  return 0;
}
