/*
 * pht_psis.h — specification of Pareto-smoothed importance-sampling
 * leave-one-out cross-validation (PSIS-LOO; Vehtari, Gelman, Gabry 2017;
 * Vehtari, Simpson, Gelman, Yao, Gabry 2024) of one observation from the
 * log-likelihoods l_d = log p(y | theta_d) of the usable posterior draws,
 * shared by the HIP kernel (phasetype_amd/csrc/pht_psis.hip) and the tests'
 * CPU restatement (tests/psis_spec.c).  No reference counterpart.
 *
 * Every operation is explicit (nothing contracted: every translation unit that
 * includes this is compiled with -ffp-contract=off), exp and log are
 * include/pht_detmath.h's, sqrt and / the correctly rounded ones, and every
 * sum has one written order, so a GPU wavefront and the CPU loop give the same
 * bits.  pht_psis_obs below is the whole definition, written as a loop; the
 * kernel calls the same scalar pieces and follows the same orders.
 *
 * One observation, S usable draws (fill flag 0), l_d in draw order:
 *   any l_d NaN (a bad observation for that draw): outputs NaN, flag 1.
 *   nl_d = -l_d, mx = max_d nl_d, lw_d = nl_d - mx (<= 0, the largest +0).
 *   lppd = lse_d(l_d) - log S.
 *   M = pht_psis_tail_len(S).  M < 5 (S < 25): no smoothing, khat = +inf,
 *   flag 2.
 *   Cutoff c = the (M + 1)-th largest lw.  Tail = every lw_d > c and as many
 *   copies of c as make M values, in ascending order; equal values are
 *   interchangeable, so ties leave the choice of elements open but neither
 *   the multiset of tail values nor c.  x_i = exp(tail_i) - exp(c).
 *   x_{M-1} == x_0: no smoothing, khat = +inf, flag 4.
 *   Generalised-Pareto fit (Zhang & Stephens 2009, as gpdfit of the loo
 *   package): pht_psis_fit.  A non-finite theta_j, khat or sigma, or
 *   sigma <= 0: no smoothing, khat = +inf, flag 8.
 *   The r-th smallest tail weight becomes min(log(q_r + exp(c)), 0), q_r the
 *   fitted quantile at (r - 0.5) / M (pht_psis_smoothed).
 *
 * The outputs are functions of mx and the multiset {lw_d} alone, so that
 * which of several tied draws is taken into the tail cannot change a bit: the
 * log-likelihood that goes with a weight is recovered from it, -(lw + mx)
 * (l_d up to its last bit).  With lw'_d the weight after smoothing,
 *   elpd = lse(lw' - (lw + mx)) - lse(lw'),
 * each lse = m + log(sum exp(v - m)), m the largest v, over this sequence of
 * terms: the draws in draw order at their position d, leaving out those in
 * the tail (lw_d > c, and of those equal to c the first M - #{lw_d > c} in
 * draw order); then the tail in ascending order at position r = 0..M-1.
 * Sum order (pht_psis_butterfly): 64 partial sums, partial p takes the terms
 * at positions d = p (mod 64) ascending and then r = p (mod 64) ascending;
 * then v[p] = v[p] + v[p ^ off] for off = 32, 16, 8, 4, 2, 1.  lppd's sum
 * takes l_d at position d in the same way.  Without smoothing there is no
 * tail part and nothing is left out.
 *
 * Caps: 25 <= S <= PHT_PSIS_MAXS (16384) draws for smoothing, so M <= 384 and
 * G <= 49 grid points (one lane each).
 */
#ifndef PHT_PSIS_H
#define PHT_PSIS_H

#include "pht_detmath.h"

#define PHT_PSIS_MAXS 16384
#define PHT_PSIS_MINS 25   /* fewer usable draws: M < 5 */
#define PHT_PSIS_MAXM 384  /* pht_psis_tail_len(PHT_PSIS_MAXS) */
#define PHT_PSIS_MAXG 49   /* pht_psis_grid(PHT_PSIS_MAXM) */

#define PHT_PSIS_F_BAD 1   /* a usable draw's l is NaN */
#define PHT_PSIS_F_SHORT 2 /* fewer than 25 usable draws */
#define PHT_PSIS_F_CONST 4 /* constant tail */
#define PHT_PSIS_F_FIT 8   /* the fit is not finite or sigma <= 0 */

/* M = min(floor(S / 5), m), m the smallest integer with m^2 >= 9 S (= ceil(3
 * sqrt S)); integers only */
PHT_HD int pht_psis_tail_len(int S) {
  int m = 0;
  while ((long long)m * m < 9ll * S) m++;
  const int q = S / 5;
  return q < m ? q : m;
}

/* G = 30 + floor(sqrt M); integers only */
PHT_HD int pht_psis_grid(int M) {
  int r = 0;
  while ((r + 1) * (r + 1) <= M) r++;
  return 30 + r;
}

/* index of xs: floor(M / 4 + 0.5) - 1 */
PHT_HD int pht_psis_xs_index(int M) { return (M + 2) / 4 - 1; }

PHT_HD double pht_psis_log1p(double z) {
  const double u = 1.0 + z;
  return (u == 1.0) ? z : pht_log(u) * z / (u - 1.0);
}

PHT_HD double pht_psis_expm1(double z) {
  const double u = pht_exp(z);
  if (u == 1.0) return z;
  const double um1 = u - 1.0;
  return (um1 == -1.0) ? -1.0 : um1 * z / pht_log(u);
}

/* theta_j, j = 1..G */
PHT_HD double pht_psis_theta(int G, int j, double xmax, double xs) {
  return 1.0 / xmax + (1.0 - sqrt((double)G / ((double)j - 0.5))) / 3.0 / xs;
}

/* (sum_i log1p(-theta x_i)) / M, the sum sequential in i from 0 */
PHT_HD double pht_psis_prof(double theta, const double *x, int M) {
  double acc = 0.0;
  for (int i = 0; i < M; i++) acc = acc + pht_psis_log1p(-theta * x[i]);
  return acc / (double)M;
}

PHT_HD double pht_psis_L(int M, double theta, double k) {
  return (double)M * (pht_log(-theta / k) - k - 1.0);
}

/* w_j = 1 / sum_j' exp(L_j' - L_j), sequential in j'; j0 = j - 1 */
PHT_HD double pht_psis_weight(int G, const double *L, int j0) {
  double acc = 0.0;
  const double Lj = L[j0];
  for (int q = 0; q < G; q++) acc = acc + pht_exp(L[q] - Lj);
  return 1.0 / acc;
}

/* from theta_hat = sum_j theta_j w_j (sequential in j): k, sigma and khat;
 * returns 1 when the fit may be used */
PHT_HD int pht_psis_fit_finish(int M, double theta_hat, const double *x, double *khat, double *sigma) {
  const double k = pht_psis_prof(theta_hat, x, M);
  const double sg = -k / theta_hat;
  const double kh = (k * (double)M + 5.0) / ((double)M + 10.0);
  *khat = kh;
  *sigma = sg;
  return (fabs(kh) < INFINITY) && (sg > 0.0) && (sg < INFINITY);
}

/* the whole fit over the ascending x[0..M); returns 1 when it may be used */
PHT_HD int pht_psis_fit(int M, const double *x, double *khat, double *sigma) {
  const int G = pht_psis_grid(M);
  const double xmax = x[M - 1], xs = x[pht_psis_xs_index(M)];
  double th[PHT_PSIS_MAXG], L[PHT_PSIS_MAXG];
  int ok = 1;
  for (int j = 1; j <= G; j++) {
    th[j - 1] = pht_psis_theta(G, j, xmax, xs);
    ok = ok && (fabs(th[j - 1]) < INFINITY);
    L[j - 1] = pht_psis_L(M, th[j - 1], pht_psis_prof(th[j - 1], x, M));
  }
  double theta_hat = 0.0;
  for (int j = 0; j < G; j++) theta_hat = theta_hat + th[j] * pht_psis_weight(G, L, j);
  return pht_psis_fit_finish(M, theta_hat, x, khat, sigma) && ok;
}

/* the smoothed r-th smallest tail weight, r = 1..M; ec = exp(c) */
PHT_HD double pht_psis_smoothed(int r, int M, double khat, double sigma, double ec) {
  const double p = ((double)r - 0.5) / (double)M;
  const double Lp = -pht_psis_log1p(-p);
  const double q = (khat == 0.0) ? sigma * Lp : sigma * pht_psis_expm1(khat * Lp) / khat;
  return fmin(pht_log(q + ec), 0.0);
}

/* the 64 partial sums into one */
PHT_HD double pht_psis_butterfly(const double *part) {
  double v[64], w[64];
  for (int p = 0; p < 64; p++) v[p] = part[p];
  for (int off = 32; off >= 1; off >>= 1) {
    for (int p = 0; p < 64; p++) w[p] = v[p] + v[p ^ off];
    for (int p = 0; p < 64; p++) v[p] = w[p];
  }
  return v[0];
}

/* ascending heap sort (the definition needs the order statistics only; the
 * kernel selects them without sorting the draws) */
PHT_HD void pht_psis_sift(double *a, int root, int end) {
  for (;;) {
    int ch = 2 * root + 1;
    if (ch >= end) return;
    if (ch + 1 < end && a[ch + 1] > a[ch]) ch++;
    if (!(a[ch] > a[root])) return;
    const double t = a[ch];
    a[ch] = a[root];
    a[root] = t;
    root = ch;
  }
}
PHT_HD void pht_psis_sort(double *a, int n) {
  for (int start = n / 2 - 1; start >= 0; start--) pht_psis_sift(a, start, n);
  for (int end = n - 1; end > 0; end--) {
    const double t = a[end];
    a[end] = a[0];
    a[0] = t;
    pht_psis_sift(a, 0, end);
  }
}

/* One observation.  l[S]: the usable draws' log-likelihoods in draw order,
 * 1 <= S <= PHT_PSIS_MAXS; work: 2 S doubles. */
PHT_HD void pht_psis_obs(int S, const double *l, double *work, double *elpd, double *khat, double *lppd,
                         int *flag) {
  double *lw = work, *srt = work + S;
  double tail[PHT_PSIS_MAXM], x[PHT_PSIS_MAXM], sm[PHT_PSIS_MAXM], part[64], partb[64];
  for (int d = 0; d < S; d++)
    if (l[d] != l[d]) {
      *elpd = *khat = *lppd = NAN;
      *flag = PHT_PSIS_F_BAD;
      return;
    }
  double mx = -l[0], ml = l[0];
  for (int d = 1; d < S; d++) {
    mx = fmax(mx, -l[d]);
    ml = fmax(ml, l[d]);
  }
  for (int d = 0; d < S; d++) lw[d] = (-l[d]) - mx;
  for (int p = 0; p < 64; p++) part[p] = 0.0;
  for (int d = 0; d < S; d++) part[d & 63] = part[d & 63] + pht_exp(l[d] - ml);
  *lppd = (ml + pht_log(pht_psis_butterfly(part))) - pht_log((double)S);

  const int M = pht_psis_tail_len(S);
  int fl = 0, smooth = 0, ntie = 0;
  double c = 0.0, kh = INFINITY, sg = 0.0;
  if (M < 5) {
    fl = PHT_PSIS_F_SHORT;
  } else {
    for (int d = 0; d < S; d++) srt[d] = lw[d];
    pht_psis_sort(srt, S);
    c = srt[S - M - 1];
    const double ec = pht_exp(c);
    int cg = 0;
    for (int i = 0; i < M; i++) {
      tail[i] = srt[S - M + i];
      cg += tail[i] > c;
      x[i] = pht_exp(tail[i]) - ec;
    }
    ntie = M - cg;
    if (x[M - 1] == x[0]) {
      fl = PHT_PSIS_F_CONST;
    } else if (!pht_psis_fit(M, x, &kh, &sg)) {
      fl = PHT_PSIS_F_FIT;
      kh = INFINITY;
    } else {
      smooth = 1;
      for (int r = 1; r <= M; r++) sm[r - 1] = pht_psis_smoothed(r, M, kh, sg, ec);
    }
  }
  /* the two sums of elpd: the largest terms, then the partial sums */
  double ma = -INFINITY, mb = -INFINITY;
  for (int pass = 0; pass < 2; pass++) {
    int seen = 0;
    for (int p = 0; p < 64; p++) part[p] = partb[p] = 0.0;
    for (int d = 0; d < S; d++) {
      if (smooth && (lw[d] > c || (lw[d] == c && seen++ < ntie))) continue;
      const double b = lw[d], a = lw[d] - (lw[d] + mx);
      if (pass == 0) {
        ma = fmax(ma, a);
        mb = fmax(mb, b);
      } else {
        part[d & 63] = part[d & 63] + pht_exp(a - ma);
        partb[d & 63] = partb[d & 63] + pht_exp(b - mb);
      }
    }
    for (int r = 0; smooth && r < M; r++) {
      const double b = sm[r], a = sm[r] - (tail[r] + mx);
      if (pass == 0) {
        ma = fmax(ma, a);
        mb = fmax(mb, b);
      } else {
        part[r & 63] = part[r & 63] + pht_exp(a - ma);
        partb[r & 63] = partb[r & 63] + pht_exp(b - mb);
      }
    }
  }
  *elpd = (ma + pht_log(pht_psis_butterfly(part))) - (mb + pht_log(pht_psis_butterfly(partb)));
  *khat = kh;
  *flag = fl;
}

#endif /* PHT_PSIS_H */
