/*
 * pht_loglik.h — specification of the observed-data log-likelihood of a
 * posterior draw, shared by the HIP kernel (phasetype_amd/csrc/pht_loglik.hip),
 * the host (host_loglik.cpp) and the tests' CPU restatement
 * (tests/loglik_spec.c).
 *
 * For a draw theta -> (S, s) with S = Q diag(lambda) Q^-1 and pi = e_1 (as in
 * every kernel here, src/PHT_MCMC_Aslett.c:279-297):
 *   exact observation     f(y)    = pi exp(S y) s = sum_i a_i exp(lambda_i y)
 *   censored observation  Fbar(y) = pi exp(S y) 1 = sum_i b_i exp(lambda_i y)
 *   a_i = piQ_i (Q^-1 s)_i,  b_i = piQ_i (Q^-1 1)_i,  piQ_i = Q[0, i]
 * (built on the host by pht_loglik_build; Q^-1 s and Q^-1 1 are solved
 * against Q, so that sum_i a_i = s_1 and sum_i b_i = 1 hold to rounding).
 * The sum is taken with the largest eigenvalue factored out,
 *   l = lmax y + log sum_i c_i exp((lambda_i - lmax) y),
 * so the far tail stays finite (the unshifted sum underflows to log 0).
 *
 * Only real spectra are evaluated.  A draw whose dgeevx fails, whose spectrum
 * has a non-zero imaginary part, whose generator is not finite or whose
 * coefficients are ill-conditioned (below) carries a non-zero flag word and
 * is never evaluated: its log-likelihood is reported as NaN.
 *
 * Contract.  The sum cancels: with A = sum_i |c_i| e_i / sum_i c_i e_i,
 * e_i = exp((lambda_i - lmax) y), the rounding of the terms alone moves l by
 * about 2^-52 A, and the coefficients of a defective or nearly defective
 * spectrum (repeated or nearly equal rates: Erlang, a Coxian with one shared
 * rate) are large with alternating signs.  Nothing in LAPACK's return says so.
 * For every draw and observation the evaluator therefore returns one of two
 * things: a value l with
 *   |l - truth| <= E(A, l) = G 2^-52 A + 1e-13 |l| + ulp(l),
 * or the report that there is none: the draw is flagged (value NaN), or the
 * observation is bad for this draw (counted in nbad, pointwise NaN).  A finite
 * value outside the bound is never returned.  The guard, per observation
 * (pht_ll_finish): accabs = sum_i |c_i| e_i is accumulated beside acc, and the
 * observation is bad when G 2^-52 accabs > E_max acc.  Per draw
 * (pht_ll_illcond, in pht_loglik_build): the survival sum at y = 0, where the
 * truth is 1, is already past the guard, G 2^-52 sum_i |b_i| > E_max, or a
 * coefficient of a finite generator is not finite: PHT_LL_F_ILLCOND.
 * G = PHT_LL_G and E_max = PHT_LL_EMAX are measured.
 * acc and the bits of every accepted l do not depend on the guard.
 *
 * Every operation is explicit (fma where written, nothing else contracted:
 * every translation unit that includes this is compiled with
 * -ffp-contract=off), exp and log are include/pht_detmath.h's, so a GPU lane
 * and the CPU restatement give the same bits.
 */
#ifndef PHT_LOGLIK_H
#define PHT_LOGLIK_H

#include "pht_detmath.h"

/* ---- per-draw block: 64-bit words [flag][lmax][dl n][a n][b n] ---------- */
#define PHT_LL_FLAG 0
#define PHT_LL_LMAX 1
#define PHT_LL_DL 2
PHT_HD int pht_ll_words(int n) { return 2 + 3 * n; }
PHT_HD int pht_ll_off_a(int n) { return PHT_LL_DL + n; }
PHT_HD int pht_ll_off_b(int n) { return PHT_LL_DL + 2 * n; }

/* flag word (0 = usable) */
#define PHT_LL_F_INFO 1u      /* dgeevx / dgetrf / dgetri reported info != 0 */
#define PHT_LL_F_COMPLEX 2u   /* an eigenvalue with a non-zero imaginary part */
#define PHT_LL_F_NONFINITE 4u /* a non-finite entry of the generator, or eigenvalue */
/* (8u is PHT_LL_F_MU of include/pht_loglik_unif.h) */
#define PHT_LL_F_ILLCOND 16u  /* coefficients past the cancellation guard at y = 0, or not finite */

/* the cancellation guard: an observation is bad when
 * (G 2^-52) accabs > E_max acc.  G: 4 times the worst
 * (error - 1e-13 |l| - ulp(l)) / (2^-52 A) measured over the accepted values
 * of tests/test_loglik.py, 90.1.  E_max: the largest power of two at or below
 * 1e-6.  (DESIGN.md 5d has the figures.) */
#define PHT_LL_G 361.0
#define PHT_LL_EMAX 0x1p-20
#define PHT_LL_GEPS (PHT_LL_G * 0x1p-52)

/* totals per draw: int64 words [H, F, nbad, nobs] */
#define PHT_LL_TOT 4
/* an observation with |l| >= 2^40 counts as bad */
#define PHT_LL_HMAX 1099511627776.0
#define PHT_LL_FSCALE 4294967296.0 /* 2^32 */

/* one term of the shifted sum: acc + c exp(dl y) */
PHT_HD double pht_ll_expterm(double dl, double y) { return pht_exp(dl * y); }

/* the draw's flag from its survival coefficients: at y = 0 every e_i is 1 and
 * the truth is 1, so the guard reads (G 2^-52) sum_i |b_i| > E_max (i
 * increasing; a NaN or infinite sum is past it too) */
PHT_HD int pht_ll_illcond(int n, const double *b) {
  double sabs = 0.0;
  for (int i = 0; i < n; i++) sabs = sabs + fabs(b[i]);
  return !(PHT_LL_GEPS * sabs <= PHT_LL_EMAX);
}

/* l from the finished sums; *bad = 1 when the observation is bad for this
 * draw (acc <= 0, acc or l not finite, |l| >= 2^40, or the sum cancelled past
 * the guard: (G 2^-52) accabs > E_max acc), and the value is NaN */
PHT_HD double pht_ll_finish(double lmax, double y, double acc, double accabs, int *bad) {
  const int ok_acc = (acc > 0.0) && (acc < INFINITY) && (PHT_LL_GEPS * accabs <= PHT_LL_EMAX * acc);
  const double l = fma(lmax, y, pht_log(ok_acc ? acc : 1.0));
  const int ok = ok_acc && (fabs(l) < PHT_LL_HMAX);
  *bad = !ok;
  return ok ? l : NAN;
}

/* l(y | draw) for one observation from one block (n <= 32) */
PHT_HD double pht_ll_eval(int n, const double *blk, double y, int cens, int *bad) {
  const double *dl = blk + PHT_LL_DL;
  const double *c = blk + (cens ? pht_ll_off_b(n) : pht_ll_off_a(n));
  double acc = 0.0, accabs = 0.0;
  for (int i = 0; i < n; i++) {
    const double e = pht_ll_expterm(dl[i], y);
    acc = fma(c[i], e, acc);
    accabs = fma(fabs(c[i]), e, accabs);
  }
  return pht_ll_finish(blk[PHT_LL_LMAX], y, acc, accabs, bad);
}

/* fixed-point words of a finite l, |l| < 2^40: l = h + f 2^-32 up to 2^-33 */
PHT_HD void pht_ll_fixed(double l, long long *h, long long *f) {
  const double hd = rint(l);
  *h = (long long)hd;
  *f = llrint((l - hd) * PHT_LL_FSCALE);
}

/* ---- WAIC accumulators: six words per observation ------------------------ */
/* all zero = no finite draw yet.  ref: the first finite l (the sums S1, S2
 * are of u = l - ref); m, r: running max and sum_d exp(l_d - m). */
typedef struct {
  double ref, S1, S2, m, r;
  long long cnt;
} pht_waic_t;

/* one finite l, in draw-index order */
PHT_HD void pht_waic_update(pht_waic_t *w, double l) {
  if (w->cnt == 0) {
    w->ref = l;
    w->m = l;
    w->r = 1.0;
    w->S1 = 0.0;
    w->S2 = 0.0;
    w->cnt = 1;
    return;
  }
  const double u = l - w->ref;
  w->S1 = w->S1 + u;
  w->S2 = fma(u, u, w->S2);
  w->cnt += 1;
  const int up = l > w->m;
  const double e = pht_exp(up ? w->m - l : l - w->m);
  w->r = up ? fma(w->r, e, 1.0) : w->r + e;
  w->m = up ? l : w->m;
}

#endif /* PHT_LOGLIK_H */
