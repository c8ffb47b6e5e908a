/*
 * pht_forecast.h — specification of the fleet forecast: for every posterior
 * draw (S, s) with pi = e_1, every unit still in service at age c_i (a
 * right-censored observation) and every horizon h_j, the conditional failure
 * probability
 *   q = P(T <= c_i + h_j | T > c_i) = 1 - Fbar(c_i + h_j) / Fbar(c_i),
 * its exact sums over the units per draw and its sum over the draws per unit.
 * The per-observation counterpart of include/pht_quantile.h's residual life
 * of one age.  No reference counterpart.  Shared by the HIP kernel
 * (phasetype_amd/csrc/pht_forecast.hip), the host (host_forecast.cpp) and the
 * tests' CPU restatement (tests/forecast_spec.c).
 *
 * Per draw.  The meta words of pht_llu_meta and the table of pht_llu_table
 * (include/pht_loglik_unif.h, unchanged), sized for
 *   y_max = pht_fc_ymax(ymax_c, h_max) = ymax_c + h_max,
 * ymax_c the largest CENSORED observation of the context and h_max the last
 * horizon.  The evaluator's limits are inherited: pi = e_1 and K <= 2047, so
 * mu (c + h) up to roughly 1500.  A draw flagged by pht_llu_meta
 * (PHT_LL_F_NONFINITE, PHT_LL_F_MU: loglik_unif's flag words) is skipped: its
 * words are zero, its pointwise values NaN, and no unit's qsum or cnt moves.
 *
 * Per (draw, unit, horizon), horizons in ascending order:
 *   l0 = pht_llu_eval(.., y = c_i, cens = 1, ..)        once per (draw, unit)
 *   lj = pht_llu_eval(.., y = c_i + h_j, cens = 1, ..)
 *   dl = lj - l0,   q = pht_fc_q(dl).
 * A unit whose evaluation at c_i or at c_i + h_j is bad is BAD for that
 * (draw, horizon): counted (nbad), never summed, pointwise NaN.  h_j = 0
 * evaluates the same y twice, so dl = 0 and q = 0 exactly.
 *
 * pht_fc_q(dl) = -expm1(dl) without cancellation.  dl >= 0 gives 0: the truth
 * is non-increasing in y, so a positive difference is rounding.  For
 * dl > PHT_FC_THRESH = -0.25:  q = -(dl P(dl)),  P(x) = sum_{k=0..13}
 * x^k / (k + 1)!  by Horner in fma (PHT_FC_DEG = 13; the first term left out
 * is below 0.25^14 / 15! = 2.9e-21).  Otherwise q = 1 - pht_exp(dl) (at
 * dl <= -0.25, e^dl <= 0.78 and the difference keeps its digits).
 * Measured relative error of the function itself against mpmath (60 digits;
 * the grid of tests/test_forecast.py at ten times its density, 200 102 points:
 * -10^-300 .. -700 log-uniformly, -10^-3 .. -10 and -0.2 .. -0.3 densely, the
 * 50 doubles on either side of the threshold): 1.50 x 2^-53 in the polynomial's range,
 * 2.26 x 2^-53 in that of 1 - exp (2^-53 relative is between half an ulp and
 * one ulp of the result), so
 *   r = PHT_FC_R = 3 * 2^-53
 * covers both.  The function is monotone (non-increasing in dl) up to that
 * error: two arguments whose true values differ by more than 2 r q are
 * ordered, in particular any two at least 2^-44 apart on either side of the
 * threshold; adjacent doubles may differ by one ulp the wrong way.
 *
 * Contract.  With b(y) the evaluator's bound at y (2^-53 (n + 9) (k_hi + 1) +
 * 2^-56 + ulp(l)), e = b(c_i) + b(c_i + h) + ulp(dl) bounds |dl - dl_true|,
 * and since 1 - q^ = e^dl (1 + ..):
 *   |q^ - q| <= (1 - q) expm1(e) + r q
 * (q the truth; for the clamped case dl >= 0 the truth satisfies q <=
 * expm1(e), which the first term covers).
 *
 * Exact reductions.  Per draw and horizon four int64 words [M, V, nbad,
 * nunits] (PHT_FC_WORDS), over the units that are good for that draw and
 * horizon:
 *   M = sum_i llrint(q 2^40),   V = sum_i llrint((q (1 - q)) 2^40),
 * the mean and the variance, in units of 2^-40, of that draw's Poisson-
 * binomial failure count; nbad and nunits count the bad and the good units.
 * At most PHT_FC_MAXUNITS = 2^22 censored units per context, so every sum is
 * at most 2^62.  Integer sums: they depend on neither the grid, the batch nor
 * the shard, and shards and ranks add them like loglik_unif's words.
 *
 * Per unit and horizon: qsum, the sum of q over the draws in which the unit
 * was good, IN DRAW ORDER (qsum <- qsum + q), and cnt, how many those were.
 *
 * Limits: 1 <= nh <= PHT_FC_MAXH = 16 horizons, each finite, >= 0, strictly
 * increasing (pht_fc_horizons_ok).
 *
 * Every operation is explicit; every unit that includes this is compiled with
 * -ffp-contract=off; exp and log are include/pht_detmath.h's.  A GPU lane and
 * the CPU restatement give the same bits.
 */
#ifndef PHT_FORECAST_H
#define PHT_FORECAST_H

#include "pht_loglik_unif.h"

#define PHT_FC_MAXH 16              /* horizons of a call */
#define PHT_FC_MAXUNITS (1L << 22)  /* censored units of a context */
#define PHT_FC_SCALE 0x1p40         /* the fixed point of M and V */
#define PHT_FC_THRESH (-0.25)       /* above: the polynomial; at or below: 1 - exp */
#define PHT_FC_DEG 13               /* degree of P */
#define PHT_FC_R (3.0 * 0x1p-53)    /* measured relative error bound of pht_fc_q */

#define PHT_FC_WORDS 4 /* [M, V, nbad, nunits] per (draw, horizon) */
#define PHT_FC_W_M 0
#define PHT_FC_W_V 1
#define PHT_FC_W_NBAD 2
#define PHT_FC_W_NUNITS 3

/* the y the draw's table is sized for */
PHT_HD double pht_fc_ymax(double ymax_c, double hmax) { return ymax_c + hmax; }

/* 1 <= nh <= 16, every horizon finite and >= 0, strictly increasing */
PHT_HD int pht_fc_horizons_ok(int nh, const double *h) {
  if (nh < 1 || nh > PHT_FC_MAXH) return 0;
  for (int j = 0; j < nh; j++) {
    if (!(h[j] >= 0.0) || !(h[j] < INFINITY)) return 0;
    if (j && !(h[j] > h[j - 1])) return 0;
  }
  return 1;
}

/* -expm1(dl) for a finite or -inf dl; 0 for dl >= 0 */
PHT_HD double pht_fc_q(double dl) {
  /* 1 / (k + 1)!, k = 13 .. 1 (Horner from the top; the k = 0 coefficient is 1) */
  double p = 1.0 / 87178291200.0;
  p = fma(p, dl, 1.0 / 6227020800.0);
  p = fma(p, dl, 1.0 / 479001600.0);
  p = fma(p, dl, 1.0 / 39916800.0);
  p = fma(p, dl, 1.0 / 3628800.0);
  p = fma(p, dl, 1.0 / 362880.0);
  p = fma(p, dl, 1.0 / 40320.0);
  p = fma(p, dl, 1.0 / 5040.0);
  p = fma(p, dl, 1.0 / 720.0);
  p = fma(p, dl, 1.0 / 120.0);
  p = fma(p, dl, 1.0 / 24.0);
  p = fma(p, dl, 1.0 / 6.0);
  p = fma(p, dl, 0.5);
  p = fma(p, dl, 1.0);
  const double small = -(dl * p);
  const double large = 1.0 - pht_exp(dl);
  const double q = (dl > PHT_FC_THRESH) ? small : large;
  return (dl >= 0.0) ? 0.0 : q;
}

/* the fixed-point words of one q in [0, 1] */
PHT_HD void pht_fc_fixed(double q, long long *m, long long *v) {
  *m = llrint(q * PHT_FC_SCALE);
  *v = llrint((q * (1.0 - q)) * PHT_FC_SCALE);
}

/* q of one (unit, horizon) from the two evaluations, l0 at c_i and lj at
 * c_i + h_j, and their bad flags; *bad = 1 and NaN for a bad cell */
PHT_HD double pht_fc_pair(double l0, int bad0, double lj, int badj, int *bad) {
  const int b = bad0 | badj;
  const double dl = (b ? 0.0 : lj) - (b ? 0.0 : l0);
  const double q = pht_fc_q(dl);
  *bad = b;
  return b ? NAN : q;
}

/* the y of the evaluations of one unit: j = -1 the age itself, j >= 0 the age
 * plus horizon j */
PHT_HD double pht_fc_y(double c, const double *h, int j) { return (j < 0) ? c : c + h[(j < 0) ? 0 : j]; }

/* The whole specification for one draw on the host (no device): ncens units
 * of ages c, nh horizons (pht_fc_horizons_ok), the table sized for
 * pht_fc_ymax(ymax_c, h[nh - 1]).  words: [nh][PHT_FC_WORDS], written (zero
 * for a flagged draw).  qsum, cnt: [ncens][nh], UPDATED (the draws of a chain
 * in order: one call each); q: [ncens][nh], written (NaN where bad); each of
 * the three may be null.  tab: room for 2 (PHT_LLU_MAXK + 1) doubles, invk:
 * for PHT_LLU_MAXK + 1.  Returns the draw's flag word. */
PHT_HD unsigned pht_fc_draw(int n, const double *S, const double *s, long ncens, const double *c, double ymax_c,
                            int nh, const double *h, double *tab, double *invk, long long *words, double *qsum,
                            long long *cnt, double *q) {
  double meta[PHT_LLU_META];
  const unsigned flag = pht_llu_meta(n, S, s, pht_fc_ymax(ymax_c, h[nh - 1]), meta);
  for (int j = 0; j < nh * PHT_FC_WORDS; j++) words[j] = 0;
  if (flag) {
    if (q)
      for (long k = 0; k < ncens * nh; k++) q[k] = NAN;
    return flag;
  }
  const int K = (int)meta[PHT_LLU_M_K];
  const double mu = meta[PHT_LLU_M_MU], abar = meta[PHT_LLU_M_ABAR];
  pht_llu_table(n, S, s, mu, K, tab);
  for (int k = 0; k <= K; k++) invk[k] = k ? 1.0 / (double)k : 0.0;
  for (long i = 0; i < ncens; i++) {
    int bad0 = 0;
    double l0 = 0.0;
    for (int j = -1; j < nh; j++) {
      int badj, khi, bad;
      const double lj = pht_llu_eval(tab, invk, K, mu, abar, pht_fc_y(c[i], h, j), 1, &badj, &khi);
      if (j < 0) {
        l0 = lj;
        bad0 = badj;
        continue;
      }
      const double qv = pht_fc_pair(l0, bad0, lj, badj, &bad);
      long long *w = words + j * PHT_FC_WORDS;
      if (bad) {
        w[PHT_FC_W_NBAD] += 1;
      } else {
        long long m, v;
        pht_fc_fixed(qv, &m, &v);
        w[PHT_FC_W_M] += m;
        w[PHT_FC_W_V] += v;
        w[PHT_FC_W_NUNITS] += 1;
        if (qsum) qsum[i * nh + j] = qsum[i * nh + j] + qv;
        if (cnt) cnt[i * nh + j] += 1;
      }
      if (q) q[i * nh + j] = qv;
    }
  }
  return flag;
}

#endif /* PHT_FORECAST_H */
