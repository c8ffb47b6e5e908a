/*
 * host_loglik.cpp — log-likelihood of posterior draws.
 *
 * No reference counterpart: the reference returns the draws and nothing
 * else.  Two evaluators, chosen per call.  Spectral (specification in
 * include/pht_loglik.h, kernel pht_loglik.hip; pht_loglik_build +
 * pht_ctx_loglik): a draw whose spectrum is complex (the sampler warns and
 * uses the real parts, as the reference does), whose LAPACK call fails,
 * whose generator is not finite or whose coefficients cancel past the guard
 * of pht_loglik.h (a defective or nearly defective spectrum: LAPACK does not
 * report those) is flagged and never evaluated; an observation whose sum
 * cancels past the guard is bad for that draw.
 * Uniformisation (include/pht_loglik_unif.h, pht_loglik_unif.hip;
 * pht_ctx_loglik_unif): any finite generator, straight from (S, s), no LAPACK.
 * pht_ctx_loo_fill / pht_ctx_loo_fill_unif are the same two calls with their
 * pointwise rows kept on the device for PSIS-LOO (host_psis.cpp).
 */
#include <math.h>
#include <string.h>

#include <cmath>

#include "host_internal.h"
#include "pht_loglik.h"
#include "pht_loglik_args.h"
#include "pht_loglik_unif.h"
#include "pht_loglik_unif_args.h"

using namespace pht;
using namespace pht::host;

/* x1 = Q^-1 r1, x2 = Q^-1 r2 by Gaussian elimination with partial pivoting
 * (column-major Q, n <= kMaxN).  Solving against Q keeps Q x - r at rounding
 * level, which is what the coefficients need: sum_i Q[0,i] x_i must give back
 * r_1 (the density at 0 is s_1, the survival 1).  eigen()'s dgetri inverse,
 * kept as the reference computes it, bounds X Q - I instead, and the
 * coefficients from it were off by ~100 cond(Q) ulps at n = 15. */
static bool solve_pair(int n, const double *Q, const double *r1, const double *r2, double *x1, double *x2) {
  std::vector<double> A(Q, Q + (size_t)n * n);
  for (int i = 0; i < n; i++) {
    x1[i] = r1[i];
    x2[i] = r2[i];
  }
  for (int k = 0; k < n; k++) {
    int p = k;
    for (int i = k + 1; i < n; i++)
      if (fabs(A[i + k * n]) > fabs(A[p + k * n])) p = i;
    if (!(fabs(A[p + k * n]) > 0.0) || !std::isfinite(A[p + k * n])) return false;
    if (p != k) {
      for (int j = 0; j < n; j++) std::swap(A[k + j * n], A[p + j * n]);
      std::swap(x1[k], x1[p]);
      std::swap(x2[k], x2[p]);
    }
    for (int i = k + 1; i < n; i++) {
      const double f = A[i + k * n] / A[k + k * n];
      for (int j = k + 1; j < n; j++) A[i + j * n] -= f * A[k + j * n];
      x1[i] -= f * x1[k];
      x2[i] -= f * x2[k];
    }
  }
  for (int k = n - 1; k >= 0; k--) {
    for (int j = k + 1; j < n; j++) {
      x1[k] -= A[k + j * n] * x1[j];
      x2[k] -= A[k + j * n] * x2[j];
    }
    x1[k] /= A[k + k * n];
    x2[k] /= A[k + k * n];
  }
  return true;
}

extern "C" int pht_loglik_bytes(int n) { return (n < 1 || n > kMaxN) ? -1 : 8 * pht_ll_words(n); }

extern "C" int pht_loglik_build(int n, const double *S, const double *s, unsigned char *out, int out_bytes) {
  if (n < 1 || n > kMaxN) {
    set_err("pht_loglik_build: n = %d outside 1..%d", n, kMaxN);
    return -1;
  }
  const int words = pht_ll_words(n);
  if (!S || !s || !out || out_bytes < 8 * words) {
    set_err("pht_loglik_build: null argument or out_bytes < %d", 8 * words);
    return -2;
  }
  if (!lapack_ready()) {
    set_err("no LAPACK bound (call pht_bind_lapack or set PHT_LAPACK_LIB)");
    return -1;
  }
  std::vector<double> w(words, 0.0), ev(n, 0.0), evi(n, 0.0), Q(n * n, 0.0), Qinv(n * n, 0.0), Qs(n, 0.0), Q1(n, 0.0);
  uint64_t flag = 0;
  bool finite = true;
  for (int k = 0; k < n * n; k++) finite = finite && std::isfinite(S[k]);
  for (int k = 0; k < n; k++) finite = finite && std::isfinite(s[k]);
  if (!finite) {
    flag |= PHT_LL_F_NONFINITE; /* (LAPACK is not asked about such a matrix) */
  } else if (eigen(n, S, ev.data(), Q.data(), Qinv.data(), evi.data()) != 0) {
    flag |= PHT_LL_F_INFO;
  } else {
    for (int i = 0; i < n; i++)
      if (evi[i] != 0.0) flag |= PHT_LL_F_COMPLEX;
    const std::vector<double> ones(n, 1.0);
    if (!solve_pair(n, Q.data(), s, ones.data(), Qs.data(), Q1.data())) flag |= PHT_LL_F_INFO;
    double lmax = ev[0];
    for (int i = 1; i < n; i++)
      if (ev[i] > lmax) lmax = ev[i];
    w[PHT_LL_LMAX] = lmax;
    for (int i = 0; i < n; i++) {
      const double piQ = Q[0 + i * n]; /* pi = e_1 */
      const double dl = ev[i] - lmax, a = piQ * Qs[i], b = piQ * Q1[i];
      if (!std::isfinite(ev[i])) flag |= PHT_LL_F_NONFINITE;
      /* (a finite generator: the solve against a singular Q overflowed) */
      if (!std::isfinite(a) || !std::isfinite(b)) flag |= PHT_LL_F_ILLCOND;
      w[PHT_LL_DL + i] = dl;
      w[pht_ll_off_a(n) + i] = a;
      w[pht_ll_off_b(n) + i] = b;
    }
    /* a defective or nearly defective spectrum: LAPACK returns info = 0 and
     * the pivots are not zero, but the survival sum cancels past the guard
     * already at y = 0 */
    if (pht_ll_illcond(n, w.data() + pht_ll_off_b(n))) flag |= PHT_LL_F_ILLCOND;
  }
  if (flag) std::fill(w.begin(), w.end(), 0.0);
  memcpy(out, w.data(), 8 * (size_t)words);
  memcpy(out + 8 * PHT_LL_FLAG, &flag, 8);
  return (int)flag;
}

/* the WAIC state of the context's observations: allocated and zeroed on
 * first use; zero: started afresh */
static int loglik_waic(pht_ctx *c, bool zero) {
  const size_t cnt = c->count;
  if (!c->obs.d_waic) {
    HIPCHK(c->obs.d_waic.alloc(5 * cnt));
    HIPCHK(c->obs.d_wcnt.alloc(cnt));
    zero = true;
  }
  if (zero) {
    HIPCHK(hipMemsetAsync(c->obs.d_waic.get(), 0, sizeof(double) * 5 * cnt, c->stream.get()));
    HIPCHK(hipMemsetAsync(c->obs.d_wcnt.get(), 0, sizeof(long long) * cnt, c->stream.get()));
  }
  return 0;
}

static int loglik_need_obs(pht_ctx *c, const char *who) {
  if (!c) {
    set_err("%s: null context", who);
    return -1;
  }
  if (c->count < 1 || !c->obs.d_y) {
    set_err("%s: no observations set on this context (pht_ctx_set_obs)", who);
    return -1;
  }
  return 0;
}

/* where a launch of either evaluator puts its results */
struct LoglikOut {
  unsigned long long *totals; /* the launch's first draw */
  double *pw;
  int acc;
  double *w_ref, *w_S1, *w_S2, *w_m, *w_r;
  long long *w_cnt;
};

/* What a call of either evaluator does around its launches: the totals, the
 * pointwise staging buffer and the WAIC state (shared by both, so calls of
 * either kind with `accumulate` continue one state), the batches in draw
 * order, the pointwise rows back in the caller's observation order, the
 * device time of the call.  launch(d0, nb, out) enqueues draws [d0, d0 + nb)
 * on the context's stream.  dev_rows (pht_ctx_loo_fill*): the kernels write
 * the pointwise rows of draw d at dev_rows + d * count instead, in the device
 * order, and nothing is staged or copied. */
template <class Launch>
static int loglik_batches(pht_ctx *c, int ndraws, int batch, long long *totals, double *pointwise, int accumulate,
                          double *dev_rows, Launch launch) {
  hipStream_t st = c->stream.get();
  const long count = c->count;
  if (cu_count(c) < 0) return -1;
  HIPCHK(ensure(c->d_lltot, (size_t)ndraws * PHT_LL_TOT));
  const int bmax = std::min(batch, ndraws);
  if (pointwise) HIPCHK(ensure(c->obs.d_llpw, (size_t)bmax * (size_t)count));
  if (accumulate && loglik_waic(c, false)) return -1;
  HIPCHK(hipMemsetAsync(c->d_lltot.get(), 0, sizeof(unsigned long long) * (size_t)ndraws * PHT_LL_TOT, st));
  std::vector<double> hpw;
  if (pointwise) hpw.resize((size_t)bmax * (size_t)count);
  /* device time of the call's launches (pointwise mode: with the copies
   * between them), read through pht_ctx_last_kernel_ms */
  HIPCHK(hipEventRecord(c->ev0.get(), st));
  for (int d0 = 0; d0 < ndraws; d0 += batch) {
    const int nb = std::min(batch, ndraws - d0);
    LoglikOut o{};
    o.totals = c->d_lltot.get() + (size_t)d0 * PHT_LL_TOT;
    o.pw = dev_rows ? dev_rows + (size_t)d0 * (size_t)count : (pointwise ? c->obs.d_llpw.get() : nullptr);
    o.acc = accumulate ? 1 : 0;
    if (accumulate) {
      o.w_ref = c->obs.d_waic.get();
      o.w_S1 = c->obs.d_waic.get() + count;
      o.w_S2 = c->obs.d_waic.get() + 2 * count;
      o.w_m = c->obs.d_waic.get() + 3 * count;
      o.w_r = c->obs.d_waic.get() + 4 * count;
      o.w_cnt = c->obs.d_wcnt.get();
    }
    if (launch(d0, nb, o)) return -1;
    if (pointwise) {
      HIPCHK(hipMemcpyAsync(hpw.data(), c->obs.d_llpw.get(), sizeof(double) * (size_t)nb * (size_t)count,
                            hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      for (int d = 0; d < nb; d++) { /* back to the caller's observation order */
        const double *src = hpw.data() + (size_t)d * count;
        double *dst = pointwise + (size_t)(d0 + d) * count;
        for (long k = 0; k < count; k++) dst[c->order[k]] = src[k];
      }
    }
  }
  HIPCHK(hipEventRecord(c->ev1.get(), st));
  HIPCHK(hipMemcpyAsync(totals, c->d_lltot.get(), sizeof(long long) * (size_t)ndraws * PHT_LL_TOT,
                        hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipEventElapsedTime(&c->last_ms, c->ev0.get(), c->ev1.get()));
  return 0;
}

/* the spectral evaluator's call (dev_rows: loglik_batches) */
static int loglik_spectral(pht_ctx *c, const char *who, int ndraws, const unsigned char *blocks, int batch,
                           long long *totals, double *pointwise, int accumulate, double *dev_rows) {
  if (ndraws < 1 || !blocks || !totals || batch < 1 || batch > kLoglikBatch) {
    set_err("%s: need ndraws >= 1, blocks, totals and 1 <= batch <= %d", who, kLoglikBatch);
    return -1;
  }
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream.get();
  ctx_drain(c);
  const int n = c->n, words = pht_ll_words(n);
  HIPCHK(ensure(c->d_llblk, (size_t)ndraws * words));
  HIPCHK(hipMemcpyAsync(c->d_llblk.get(), blocks, 8 * (size_t)ndraws * words, hipMemcpyHostToDevice, st));
  return loglik_batches(c, ndraws, batch, totals, pointwise, accumulate, dev_rows,
                        [&](int d0, int nb, const LoglikOut &o) {
    LoglikArgs a{};
    a.n = n;
    a.nd = nb;
    a.count = c->count;
    a.y = c->obs.d_y.get();
    a.cens = c->obs.d_cens.get();
    a.blocks = c->d_llblk.get() + (size_t)d0 * words;
    a.totals = o.totals;
    a.pw = o.pw;
    a.acc = o.acc;
    a.w_ref = o.w_ref;
    a.w_S1 = o.w_S1;
    a.w_S2 = o.w_S2;
    a.w_m = o.w_m;
    a.w_r = o.w_r;
    a.w_cnt = o.w_cnt;
    HIPCHK(pht_launch_loglik(&a, 4 * c->cus, st));
    return 0;
  });
}

extern "C" int pht_ctx_loglik(pht_ctx *c, int ndraws, const unsigned char *blocks, int batch, long long *totals,
                              double *pointwise, int accumulate) {
  if (loglik_need_obs(c, "pht_ctx_loglik")) return -1;
  return loglik_spectral(c, "pht_ctx_loglik", ndraws, blocks, batch, totals, pointwise, accumulate, nullptr);
}

extern "C" int pht_ctx_loglik_unif_K(pht_ctx *c, double mu) {
  if (loglik_need_obs(c, "pht_ctx_loglik_unif_K")) return -1;
  if (!(mu > 0.0) || !std::isfinite(mu)) {
    set_err("pht_ctx_loglik_unif_K: mu must be positive and finite");
    return -1;
  }
  return pht_llu_K(mu, c->ymax);
}

/* the uniformisation evaluator's call (dev_rows: loglik_batches) */
static int loglik_unif(pht_ctx *c, const char *who, int ndraws, const double *S, const double *s, int batch,
                       long long *totals, double *pointwise, int accumulate, int *flags_out, double *dev_rows) {
  if (ndraws < 1 || !S || !s || !totals || batch < 1 || batch > kLoglikBatch) {
    set_err("%s: need ndraws >= 1, S, s, totals and 1 <= batch <= %d", who, kLoglikBatch);
    return -1;
  }
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream.get();
  ctx_drain(c);
  /* the draws' meta words (flags, mu, K from the shard's largest y); the table
   * buffer holds one batch: every draw at the stride of the call's largest K */
  const UnifPlan plan(c->n, ndraws, S, s, batch, flags_out, [&](int, const double *Sd, const double *sd, double *m) {
    return pht_llu_meta(c->n, Sd, sd, c->ymax, m);
  });
  if (unif_stage(c, plan, S, s)) return -1;
  return loglik_batches(c, ndraws, batch, totals, pointwise, accumulate, dev_rows,
                        [&](int d0, int nb, const LoglikOut &o) {
    LlunifTableArgs t;
    if (unif_tables(c, plan, d0, nb, t)) return -1;
    LlunifArgs a{};
    a.nd = nb;
    a.Kmax = plan.Kmax(d0, nb);
    a.count = c->count;
    a.y = c->obs.d_y.get();
    a.cens = c->obs.d_cens.get();
    a.meta = t.meta;
    a.tab = t.tab;
    a.stride = t.stride;
    a.totals = o.totals;
    a.pw = o.pw;
    a.acc = o.acc;
    a.w_ref = o.w_ref;
    a.w_S1 = o.w_S1;
    a.w_S2 = o.w_S2;
    a.w_m = o.w_m;
    a.w_r = o.w_r;
    a.w_cnt = o.w_cnt;
    /* (under 64 KB of LDS a block: two blocks a CU, half the spectral kernel's cap) */
    HIPCHK(pht_launch_llunif(&a, 2 * c->cus, st));
    return 0;
  });
}

extern "C" int pht_ctx_loglik_unif(pht_ctx *c, int ndraws, const double *S, const double *s, int batch,
                                   long long *totals, double *pointwise, int accumulate, int *flags_out) {
  if (loglik_need_obs(c, "pht_ctx_loglik_unif")) return -1;
  return loglik_unif(c, "pht_ctx_loglik_unif", ndraws, S, s, batch, totals, pointwise, accumulate, flags_out,
                     nullptr);
}

/* ---- PSIS-LOO fills: the same calls, their pointwise rows kept on the device
 * in the context's matrix (host_psis.cpp owns it), the WAIC state untouched */
static int loo_fill_rows(pht_ctx *c, const char *who, int row0, int nd) {
  if (loglik_need_obs(c, who)) return -1;
  const auto &L = c->obs.loo;
  if (L.ndraws < 1 || !L.d_mat) {
    set_err("%s: no matrix on this context (pht_ctx_loo_begin)", who);
    return -1;
  }
  if (row0 < 0 || nd < 1 || (long long)row0 + nd > L.ndraws) {
    set_err("%s: rows [%d, %lld) outside the matrix's %d draws", who, row0, (long long)row0 + nd, L.ndraws);
    return -1;
  }
  /* unusable until the fill is through (a failed fill leaves them so) */
  std::fill(c->obs.loo.usable.begin() + row0, c->obs.loo.usable.begin() + row0 + nd, (unsigned char)0);
  return 0;
}

extern "C" int pht_ctx_loo_fill(pht_ctx *c, int row0, int nd, const unsigned char *blocks, int batch,
                                long long *totals) {
  if (loo_fill_rows(c, "pht_ctx_loo_fill", row0, nd)) return -1;
  auto &L = c->obs.loo;
  double *rows = L.d_mat.get() + (size_t)row0 * (size_t)c->count;
  if (loglik_spectral(c, "pht_ctx_loo_fill", nd, blocks, batch, totals, nullptr, 0, rows)) return -1;
  const size_t bytes = 8 * (size_t)pht_ll_words(c->n);
  for (int d = 0; d < nd; d++) {
    uint64_t flag;
    memcpy(&flag, blocks + (size_t)d * bytes + 8 * PHT_LL_FLAG, 8);
    L.usable[(size_t)row0 + d] = flag == 0;
  }
  return 0;
}

extern "C" int pht_ctx_loo_fill_unif(pht_ctx *c, int row0, int nd, const double *S, const double *s, int batch,
                                     long long *totals, int *flags_out) {
  if (loo_fill_rows(c, "pht_ctx_loo_fill_unif", row0, nd)) return -1;
  auto &L = c->obs.loo;
  double *rows = L.d_mat.get() + (size_t)row0 * (size_t)c->count;
  std::vector<int> flags(nd, 0);
  if (loglik_unif(c, "pht_ctx_loo_fill_unif", nd, S, s, batch, totals, nullptr, 0, flags.data(), rows)) return -1;
  for (int d = 0; d < nd; d++) {
    L.usable[(size_t)row0 + d] = flags[d] == 0;
    if (flags_out) flags_out[d] = flags[d];
  }
  return 0;
}

extern "C" int pht_ctx_loglik_reset(pht_ctx *c) {
  if (loglik_need_obs(c, "pht_ctx_loglik_reset")) return -1;
  HIPCHK(hipSetDevice(c->device));
  return loglik_waic(c, true);
}

extern "C" int pht_ctx_loglik_state(pht_ctx *c, double *ref, double *S1, double *S2, double *m, double *r, int *cnt) {
  if (loglik_need_obs(c, "pht_ctx_loglik_state")) return -1;
  if (!ref || !S1 || !S2 || !m || !r || !cnt) {
    set_err("pht_ctx_loglik_state: null output");
    return -1;
  }
  HIPCHK(hipSetDevice(c->device));
  if (loglik_waic(c, false)) return -1;
  hipStream_t st = c->stream.get();
  const long count = c->count;
  std::vector<double> h(5 * (size_t)count);
  std::vector<long long> hc(count);
  HIPCHK(hipMemcpyAsync(h.data(), c->obs.d_waic.get(), sizeof(double) * 5 * (size_t)count, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hc.data(), c->obs.d_wcnt.get(), sizeof(long long) * (size_t)count, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  double *outs[5] = {ref, S1, S2, m, r};
  for (long k = 0; k < count; k++) {
    const long o = c->order[k];
    for (int q = 0; q < 5; q++) outs[q][o] = h[(size_t)q * count + k];
    cnt[o] = (int)hc[k];
  }
  return 0;
}
