/*
 * pht_loglik_unif.h — specification of the log-likelihood of a posterior draw
 * by uniformisation: the second evaluator of l(y | S, s), for generators whose
 * spectrum is complex or defective (where include/pht_loglik.h's spectral sum
 * does not apply) and the conditioning-free cross-check for the others.
 * Shared by the HIP kernels (phasetype_amd/csrc/pht_loglik_unif.hip), the host
 * (host_loglik.cpp) and the tests' CPU restatement (tests/loglik_unif_spec.c).
 *
 * With pi = e_1, mu = max_i -S_ii and R = I + S / mu (a sub-stochastic
 * matrix):
 *   f(y)    = pi exp(S y) s = sum_k Pois(k; mu y) ax_k,  ax_k = (R^k s)_1
 *   Fbar(y) = pi exp(S y) 1 = sum_k Pois(k; mu y) ac_k,  ac_k = (R^k 1)_1
 * Every term is non-negative: no cancellation, and an error bound that does
 * not know the eigenvector conditioning,
 *   |l - truth| <= 2^-53 (n + 9) (k_hi + 1) + 2^-56 + ulp(l),
 * k_hi the upper end of the observation's summation window.  (The ulp(l) is
 * the rounding of l itself to a double, which the series' bound does not
 * know: at a tiny y, where k_hi is small and |l| large, it is the larger
 * part.  Erlang(3), exact, y = 1e-9: l = -41.35 and k_hi = 2, the series' bound
 * 4.0e-15, one ulp 7.1e-15, and with the rates 1e-12 apart the error is 1.3
 * times the series' bound.)
 *
 * Per draw (pht_llu_meta, pht_llu_table): mu = max_i -S_ii (i increasing, from
 * 0), rinv = 1 / mu, R_ij = S_ij rinv, R_ii = fma(S_ii, rinv, 1) (as in
 * csrc/pht_unif.h).  The BACKWARD vectors B_0 = s, C_0 = 1,
 *   B_k[i] = sum_j fma(R_ij, B_{k-1}[j], .)   (j increasing, from 0; C alike),
 * sequentially in k (no doubling); the table row is (ax_k, ac_k) =
 * (B_k[0], C_k[0]), interleaved, k = 0..K, with
 *   K = min(PHT_LLU_MAXK, ceil(mu y_max + 14 sqrt(mu y_max) + 64)),
 * y_max the context's largest observation (the sampler's sizing rule and cap).
 * abar_x = max_j s_j and abar_c = 1 bound the columns from above.  Draw flags:
 * a non-finite entry of S or s sets PHT_LL_F_NONFINITE, a mu that is not
 * positive and finite PHT_LL_F_MU; a flagged draw is never evaluated (words
 * zero, pointwise NaN), like a flagged spectral block.
 *
 * Per observation and draw (pht_llu_eval; a = the ax column for an exact
 * observation, ac for a censored one, abar accordingly): lam = mu y,
 * k0 = min(floor(lam), K), il = 1 / lam.  Poisson weights relative to the
 * mode, w_k0 = 1: num = a[k0], den = 1, then
 *   downward from k0:  w <- w (k il), k <- k - 1, num = fma(w, a[k], num),
 *                      den = den + w, down to k = 0;
 *   upward from k0:    k <- k + 1, w <- w (lam invk[k]), the same two sums;
 * each direction stops BEFORE adding the term for which both hold:
 *   w < 2^-60              (the Poisson normaliser den is complete) and
 *   w u < 2^-60 num        (the numerator is complete: a_k decays like rho^k,
 *                           so in the far tail the sum's mode lies well below
 *                           the Poisson mode, and with a structural zero
 *                           s_1 = 0 the first non-zero term can lie beyond the
 *                           Poisson window at a tiny y),
 * u an upper bound of every term still to come: downward u = abar; upward
 * u = abar ac_k, since B_k <= abar_x C_k elementwise and ac is non-increasing
 * (a_j <= abar ac_k for j >= k).  The plain abar is valid upward too but asks
 * for rows the sizing rule does not provide: at ring(5), y = 200 (lam = 800,
 * K = 1260, l = -107) num is 2^-148 and w abar falls below 2^-60 num only near
 * k = 1350, while w abar ac_k does at the Poisson window's end.
 * If the upward sweep is at k = K and the rule has not been met, the table is
 * too short: the observation is BAD for this draw (counted, not summed).
 *   l = pht_log(num) - pht_log(den)
 * (the Fox-Glynn normalisation: no lgamma, no exp(-lam); the same w_k enter
 * both sums).  Bad as well: !(lam >= 0); num < 2^-900 or not finite (the table
 * entries that carry such a sum are near the denormal range);
 * |l| >= 2^40.  From l on everything is include/pht_loglik.h's: pht_ll_fixed,
 * the int64 totals, pht_waic_update.
 *
 * Every operation is explicit; every unit that includes this is compiled with
 * -ffp-contract=off; exp and log are include/pht_detmath.h's; divisions and
 * sqrt are IEEE.  A GPU lane and the CPU restatement give the same bits.
 */
#ifndef PHT_LOGLIK_UNIF_H
#define PHT_LOGLIK_UNIF_H

#include "pht_loglik.h"

#define PHT_LL_F_MU 8u /* mu = max_i -S_ii is not positive and finite */

#define PHT_LLU_MAXK 2047      /* last table row (= kUnifMaxK, the sampler's cap) */
#define PHT_LLU_TINY 0x1p-60   /* both stop rules */
#define PHT_LLU_FLOOR 0x1p-900 /* a smaller numerator is a bad observation */

/* per-draw words: [flag][mu][abar_x][K] (flag as a 64-bit integer, K as a double) */
#define PHT_LLU_META 4
#define PHT_LLU_M_FLAG 0
#define PHT_LLU_M_MU 1
#define PHT_LLU_M_ABAR 2
#define PHT_LLU_M_K 3

/* table rows for a largest lam = mu y_max */
PHT_HD int pht_llu_K(double mu, double ymax) {
  const double lmax = mu * ymax;
  const double kd = ceil(lmax + 14.0 * sqrt(lmax) + 64.0);
  return (kd < (double)PHT_LLU_MAXK) ? (int)kd : PHT_LLU_MAXK; /* (NaN: the cap) */
}

/* one draw's meta words from (S column-major n x n, s) and the context's
 * y_max; returns the flag word (0 = usable; else the other words are 0) */
PHT_HD unsigned pht_llu_meta(int n, const double *S, const double *s, double ymax, double *meta) {
  unsigned flag = 0;
  for (int k = 0; k < n * n; k++)
    if (!(fabs(S[k]) < INFINITY)) flag |= PHT_LL_F_NONFINITE;
  for (int k = 0; k < n; k++)
    if (!(fabs(s[k]) < INFINITY)) flag |= PHT_LL_F_NONFINITE;
  double mu = 0.0, abar = s[0];
  for (int i = 0; i < n; i++) {
    const double v = -S[i + i * n];
    mu = (v > mu) ? v : mu;
    abar = (s[i] > abar) ? s[i] : abar;
  }
  if (!flag && !((mu > 0.0) && (mu < INFINITY))) flag |= PHT_LL_F_MU;
  meta[PHT_LLU_M_FLAG] = pht_u2d((uint64_t)flag);
  meta[PHT_LLU_M_MU] = flag ? 0.0 : mu;
  meta[PHT_LLU_M_ABAR] = flag ? 0.0 : abar;
  meta[PHT_LLU_M_K] = flag ? 0.0 : (double)pht_llu_K(mu, ymax);
  return flag;
}

/* R_ij of the uniformised chain */
PHT_HD double pht_llu_R(double Sij, double rinv, int diag) { return diag ? fma(Sij, rinv, 1.0) : Sij * rinv; }

/* the table of a usable draw, sequentially: tab[2 k] = ax_k, tab[2 k + 1] =
 * ac_k, k = 0..K (n <= 32).  The kernel runs the same recurrence with row i
 * in lane i. */
PHT_HD void pht_llu_table(int n, const double *S, const double *s, double mu, int K, double *tab) {
  double R[32 * 32], B[32], Cv[32], Bn[32], Cn[32];
  const double rinv = 1.0 / mu;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) R[i * n + j] = pht_llu_R(S[i + j * n], rinv, i == j);
  for (int i = 0; i < n; i++) {
    B[i] = s[i];
    Cv[i] = 1.0;
  }
  tab[0] = B[0];
  tab[1] = Cv[0];
  for (int k = 1; k <= K; k++) {
    for (int i = 0; i < n; i++) {
      double b = 0.0, c = 0.0;
      for (int j = 0; j < n; j++) {
        b = fma(R[i * n + j], B[j], b);
        c = fma(R[i * n + j], Cv[j], c);
      }
      Bn[i] = b;
      Cn[i] = c;
    }
    for (int i = 0; i < n; i++) {
      B[i] = Bn[i];
      Cv[i] = Cn[i];
    }
    tab[2 * k] = B[0];
    tab[2 * k + 1] = Cv[0];
  }
}

/* both conditions of the stop rule; u bounds the terms still to come */
PHT_HD int pht_llu_stop(double w, double u, double num) {
  return (w < PHT_LLU_TINY) && (w * u < PHT_LLU_TINY * num);
}

/* l(y | draw) for one observation from the draw's table (invk[k] = 1 / k,
 * k = 1..K); *bad = 1 and NaN for a bad observation; *khi = the upper end of
 * the summation window */
PHT_HD double pht_llu_eval(const double *tab, const double *invk, int K, double mu, double abar_x, double y, int cens,
                           int *bad, int *khi) {
  const double lam = mu * y;
  const int lam_ok = (lam >= 0.0);
  const double abar = cens ? 1.0 : abar_x;
  const double *a = tab + (cens ? 1 : 0);
  const int k0 = (lam_ok && lam < (double)K) ? (int)floor(lam) : K;
  const double il = 1.0 / lam;
  double num = a[2 * k0], den = 1.0, w = 1.0;
  for (int k = k0; k > 0;) {
    w = w * ((double)k * il);
    k--;
    if (pht_llu_stop(w, abar, num)) break;
    num = fma(w, a[2 * k], num);
    den = den + w;
  }
  int k = k0, tooshort = 0;
  w = 1.0;
  for (;;) {
    if (k >= K) {
      tooshort = 1;
      break;
    }
    k++;
    w = w * (lam * invk[k]);
    if (pht_llu_stop(w, abar * tab[2 * k + 1], num)) {
      k--;
      break;
    }
    num = fma(w, a[2 * k], num);
    den = den + w;
  }
  *khi = k;
  const int ok_num = (num >= PHT_LLU_FLOOR) && (num < INFINITY);
  const double l = pht_log(ok_num ? num : 1.0) - pht_log(den);
  const int ok = lam_ok && !tooshort && ok_num && (fabs(l) < PHT_LL_HMAX);
  *bad = !ok;
  return ok ? l : NAN;
}

#endif /* PHT_LOGLIK_UNIF_H */
