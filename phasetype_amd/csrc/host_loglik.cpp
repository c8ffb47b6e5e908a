/*
 * host_loglik.cpp — log-likelihood of posterior draws.
 *
 * No reference counterpart: the reference returns the draws and nothing
 * else.  Specification in include/pht_loglik.h; the kernel is
 * pht_loglik.hip.  Spectral evaluation only: a draw whose spectrum is complex
 * (the sampler warns and uses the real parts, as the reference does), whose
 * LAPACK call fails or whose coefficients are not finite is flagged and never
 * evaluated.
 */
#include <math.h>
#include <string.h>

#include <cmath>

#include "host_internal.h"
#include "pht_loglik.h"
#include "pht_loglik_args.h"

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
      if (!std::isfinite(ev[i]) || !std::isfinite(a) || !std::isfinite(b)) flag |= PHT_LL_F_NONFINITE;
      w[PHT_LL_DL + i] = dl;
      w[pht_ll_off_a(n) + i] = a;
      w[pht_ll_off_b(n) + i] = b;
    }
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

extern "C" int pht_ctx_loglik(pht_ctx *c, int ndraws, const unsigned char *blocks, int batch, long long *totals,
                              double *pointwise, int accumulate) {
  if (loglik_need_obs(c, "pht_ctx_loglik")) return -1;
  if (ndraws < 1 || !blocks || !totals || batch < 1 || batch > kLoglikBatch) {
    set_err("pht_ctx_loglik: need ndraws >= 1, blocks, totals and 1 <= batch <= %d", kLoglikBatch);
    return -1;
  }
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream.get();
  ctx_drain(c);
  const int n = c->n, words = pht_ll_words(n);
  const long count = c->count;
  if (!c->ll_grid_cap) {
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    c->ll_grid_cap = std::max(1, cus) * 4;
  }
  HIPCHK(ensure(c->d_llblk, c->llblk_cap, (size_t)ndraws * words));
  HIPCHK(ensure(c->d_lltot, c->lltot_cap, (size_t)ndraws * PHT_LL_TOT));
  const int bmax = std::min(batch, ndraws);
  if (pointwise) HIPCHK(ensure(c->obs.d_llpw, c->obs.llpw_cap, (size_t)bmax * (size_t)count));
  if (accumulate && loglik_waic(c, false)) return -1;
  HIPCHK(hipMemcpyAsync(c->d_llblk.get(), blocks, 8 * (size_t)ndraws * words, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(c->d_lltot.get(), 0, sizeof(unsigned long long) * (size_t)ndraws * PHT_LL_TOT, st));
  std::vector<double> hpw;
  if (pointwise) hpw.resize((size_t)bmax * (size_t)count);
  /* device time of the call's launches (pointwise mode: with the copies
   * between them), read through pht_ctx_last_kernel_ms */
  HIPCHK(hipEventRecord(c->ev0.get(), st));
  for (int d0 = 0; d0 < ndraws; d0 += batch) {
    const int nb = std::min(batch, ndraws - d0);
    LoglikArgs a{};
    a.n = n;
    a.nd = nb;
    a.count = count;
    a.y = c->obs.d_y.get();
    a.cens = c->obs.d_cens.get();
    a.blocks = c->d_llblk.get() + (size_t)d0 * words;
    a.totals = c->d_lltot.get() + (size_t)d0 * PHT_LL_TOT;
    a.pw = pointwise ? c->obs.d_llpw.get() : nullptr;
    a.acc = accumulate ? 1 : 0;
    if (accumulate) {
      a.w_ref = c->obs.d_waic.get();
      a.w_S1 = c->obs.d_waic.get() + count;
      a.w_S2 = c->obs.d_waic.get() + 2 * count;
      a.w_m = c->obs.d_waic.get() + 3 * count;
      a.w_r = c->obs.d_waic.get() + 4 * count;
      a.w_cnt = c->obs.d_wcnt.get();
    }
    HIPCHK(pht_launch_loglik(&a, c->ll_grid_cap, st));
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
