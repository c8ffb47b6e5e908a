/*
 * pht_estep.h — specification of the expected sufficient statistics of a
 * phase-type model given the observations (the E-step): the time in each
 * state Z_i = E[z_i | y], the transitions N_ij = E[N_ij | y] and the exits
 * E_i = E[exit from i | y], summed over a shard, by the uniformisation of
 * include/pht_loglik_unif.h.  No reference counterpart.  Shared by the HIP
 * kernels (phasetype_amd/csrc/pht_estep.hip), the host (host_estep.cpp) and
 * the tests' CPU restatement (tests/estep_spec.c).
 *
 * With mu, R and the table ax_k = (R^k s)_1, ac_k = (R^k 1)_1 of
 * pht_loglik_unif.h, the forward vectors f_0 = e_1, f_k = f_{k-1} R and
 *   Hx_k[i][j] = sum_{l=0..k} f_l[i] (R^{k-l} s)[j]   (Hc_k: 1 in place of s),
 *   H_0 = f_0 b_0^T,  H_k = H_{k-1} R^T + f_k b_0^T,
 * the posterior law of the number of uniformised events of one observation is
 * p_k = Pois(k; mu y) a_k / sum_k' Pois(k'; mu y) a_k' (a = ax exact, ac
 * censored), and with G_k = sum_obs p_k, T_k = sum_obs y p_k per class
 *   Z_i  = sum_class sum_k T_k     H_k[i][i] / ((k + 1) a_k)
 *   N_ij = sum_class sum_k G_{k+1} R_ij H_k[i][j] / a_{k+1}        (i != j)
 *   E_i  = sum_k Gx_k f_k[i] s_i / ax_k                  (exact class only)
 *   A_i  = sum_k Gc_k f_k[i] / ac_k                   (censored class only)
 * A_i is the expected number of censored observations in state i at their
 * censoring time: Z, N and E cover the path on [0, y] (what the likelihood
 * needs; sum_i Z_i = sum y), and A is what completes a censored path beyond y
 * (the sampler runs those to absorption: A (-S)^-1 more time in each state).
 * Every quantity is non-negative; the weights of Z sum to 1 over i, those of
 * E and of A to 1 over i, those of N (virtual jumps included) to k + 1 over
 * i, j.
 *
 * Two stages.
 *
 * 1. Histograms (pht_es_window, pht_es_obs), per draw and observation.  The
 * window is pht_llu_eval's, operation for operation (so l is that
 * evaluator's bit for bit), and its ends [klo, khi], k0 and num are kept.  A
 * second pass runs the same w_k recurrence from k0 (w_k0 = 1; down
 * w_{k-1} = w_k (k il); up w_k = w_{k-1} (lam invk[k]) from w_k0 = 1 again):
 *   rn = 1 / num,  p = (w_k a[k]) rn,  yr = y (1 / yscale),
 *   g = llrint(p 2^40),  t = llrint((p yr) 2^40)
 * (pht_es_fix: 0 <= p <= 1 + 2^-50 here, and for 0 <= x < 2^51 the sum
 * x + 2^52 is x rounded to the nearest integer, ties to even, in the low bits
 * of its word: one addition and one integer subtraction, llrint's value),
 * added into the draw's int64 words [class][k][G, T] (class 0 exact, 1
 * censored; PHT_ES_ROWS rows per class whatever the draw's K).  yscale is a
 * power of two >= every y of every shard, so that shards' words add.  The
 * words are integers: their sums do not depend on the order, grid, batch or
 * shard.  At most PHT_ES_MAXOBS = 2^22 observations over all shards (a word
 * then stays below 2^62).  A bad observation (pht_llu_eval's rules) is
 * counted and adds nothing; a flagged draw is skipped, its words zero.  The
 * pass also yields pht_loglik.h's fixed-point totals [H, F, nbad, nobs].
 *
 * 2. Contraction (pht_es_contract), per draw, sequential in k = 0 .. klast,
 * klast the last row with a non-zero word.  At step k, with (ax, ac) = row k
 * and (axn, acn) = row k + 1 of pht_llu_table's table, Tq = (double)word *
 * (yscale 2^-40), Gq = (double)word * 2^-40 and a coefficient 0 wherever its
 * word is 0 or its a is not positive (the term itself is zero then):
 *   czx = Tx_k / ((double)(k + 1) * ax)   czc = Tc_k / ((double)(k + 1) * ac)
 *   cnx = Gx_{k+1} / axn                  cnc = Gc_{k+1} / acn   (k < K)
 *   cex = Gx_k / ax                       cac = Gc_k / ac
 *   Z_i  = fma(czx, Hx[i][i], Z_i), then Z_i = fma(czc, Hc[i][i], Z_i)
 *   N_ij = fma(cnx, R_ij * Hx[i][j], N_ij), then fma(cnc, R_ij * Hc[i][j], .)
 *   E_i  = fma(cex, f[i] * s_i, E_i),  A_i = fma(cac, f[i], A_i)
 * and, unless k = klast, the advance
 *   fn[j]     = sum_l fma(f[l], R[l][j], .)            (l increasing, from 0)
 *   Hxn[i][j] = fma(fn[i], s_j, sum_l fma(Hx[i][l], R[j][l], .))   (l alike)
 *   Hcn[i][j] = fma(fn[i], 1.0, sum_l fma(Hc[i][l], R[j][l], .))
 * The kernel keeps one cell (i, j) per lane and follows these orders.
 *
 * Error bound.  For a statistic whose per-observation magnitude is m_o and
 * whose quantisation unit is q_o,
 *   Z: m_o = y_o, q_o = yscale;   E, A: m_o = q_o = 1 (exact / censored ones);
 *   N: m_o = q_o = khi_o + 1 (no more jumps than uniformised events),
 *   |computed - truth| <= sum_o [ W_o 2^-41 q_o
 *                                 + (4 (n + 9) (khi_o + 1) 2^-53 + 2^-56) m_o ]
 *                         + 2 (kmax + 1) 2^-53 sum_o m_o,
 * W_o = khi_o - klo_o + 1 the observation's window, kmax the largest khi.
 * First term: each word is rounded once, by at most half a unit, and every
 * weight that multiplies it lies in [0, 1] (N: in [0, k + 1]).  Second: the
 * relative rounding error of one term p_k H_k / a — a_k and H_k[i][j] come
 * from k non-negative matrix-vector steps of length n ((n + 2) k ulps each,
 * a twice: in p_k and in the coefficient), w_k from at most 2 khi roundings,
 * num from one more sum of W terms — and the window's 2^-60 truncation.
 * Third: the two fma per step of the accumulation over k, each relative to a
 * partial sum that is at most the total.  Nothing cancels, and cond(Q) does
 * not enter.
 *
 * Every operation is explicit; every unit that includes this is compiled with
 * -ffp-contract=off; divisions are IEEE.  A GPU lane and the CPU restatement
 * give the same bits.
 */
#ifndef PHT_ESTEP_H
#define PHT_ESTEP_H

#include "pht_loglik_unif.h"

#define PHT_ES_PSCALE 0x1p40                  /* words per unit of p */
#define PHT_ES_ROWS (PHT_LLU_MAXK + 1)        /* rows per class */
#define PHT_ES_WORDS (4 * PHT_ES_ROWS)        /* int64 words per draw */
#define PHT_ES_MAXOBS (1L << 22)              /* observations over all shards */

/* word q (0 = G, 1 = T) of row k, class cls (0 exact, 1 censored) */
PHT_HD int pht_es_idx(int cls, int k, int q) { return (cls * PHT_ES_ROWS + k) * 2 + q; }

/* the smallest power of two >= ymax (1 where ymax is not positive and finite) */
PHT_HD double pht_es_yscale(double ymax) {
  if (!(ymax > 0.0) || !(ymax < INFINITY)) return 1.0;
  double p = 1.0;
  while (p < ymax) p = p * 2.0;
  while (p * 0.5 >= ymax) p = p * 0.5;
  return p;
}

/* a usable yscale: a positive finite power of two */
PHT_HD int pht_es_yscale_ok(double ys) {
  if (!(ys > 0.0) || !(ys < INFINITY)) return 0;
  return (pht_d2u(ys) & 0x000fffffffffffffull) == 0 && (pht_d2u(ys) >> 52) != 0;
}

/* an observation's window for one draw */
typedef struct {
  int k0, klo, khi; /* the Poisson mode and the first and last term summed */
  double lam, il;   /* mu y and its reciprocal */
  double num;       /* sum_k w_k a_k over the window (w_k0 = 1) */
} pht_es_win_t;

/* pht_llu_eval, operation for operation, keeping the window */
PHT_HD double pht_es_window(const double *tab, const double *invk, int K, double mu, double abar_x, double y, int cens,
                            int *bad, pht_es_win_t *win) {
  const double lam = mu * y;
  const int lam_ok = (lam >= 0.0);
  const double abar = cens ? 1.0 : abar_x;
  const double *a = tab + (cens ? 1 : 0);
  const int k0 = (lam_ok && lam < (double)K) ? (int)floor(lam) : K;
  const double il = 1.0 / lam;
  double num = a[2 * k0], den = 1.0, w = 1.0;
  int klo = 0;
  for (int k = k0; k > 0;) {
    w = w * ((double)k * il);
    k--;
    if (pht_llu_stop(w, abar, num)) {
      klo = k + 1;
      break;
    }
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
  win->k0 = k0;
  win->klo = klo;
  win->khi = k;
  win->lam = lam;
  win->il = il;
  win->num = num;
  const int ok_num = (num >= PHT_LLU_FLOOR) && (num < INFINITY);
  const double l = pht_log(ok_num ? num : 1.0) - pht_log(den);
  const int ok = lam_ok && !tooshort && ok_num && (fabs(l) < PHT_LL_HMAX);
  *bad = !ok;
  return ok ? l : NAN;
}

/* the second pass's weights: w_{k-1} from w_k, and w_k from w_{k-1} */
PHT_HD double pht_es_down(double w, int k, double il) { return w * ((double)k * il); }
PHT_HD double pht_es_up(double w, int k, double lam, const double *invk) { return w * (lam * invk[k]); }

/* llrint(x) for 0 <= x < 2^51 */
PHT_HD long long pht_es_fix(double x) { return (long long)(pht_d2u(x + 0x1p52) - pht_d2u(0x1p52)); }

/* the two words of one window term */
PHT_HD void pht_es_word(double w, double ak, double rn, double yr, long long *g, long long *t) {
  const double p = (w * ak) * rn;
  *g = pht_es_fix(p * PHT_ES_PSCALE);
  *t = pht_es_fix((p * yr) * PHT_ES_PSCALE);
}

/* one good observation's second pass, added into the draw's words */
PHT_HD void pht_es_obs(const double *tab, const double *invk, const pht_es_win_t *win, double y, double yscale,
                       int cens, long long *words) {
  const double *a = tab + (cens ? 1 : 0);
  const double rn = 1.0 / win->num, yr = y * (1.0 / yscale);
  const int cls = cens ? 1 : 0;
  long long g, t;
  double w = 1.0;
  int k = win->k0;
  pht_es_word(w, a[2 * k], rn, yr, &g, &t);
  words[pht_es_idx(cls, k, 0)] += g;
  words[pht_es_idx(cls, k, 1)] += t;
  while (k > win->klo) {
    w = pht_es_down(w, k, win->il);
    k--;
    pht_es_word(w, a[2 * k], rn, yr, &g, &t);
    words[pht_es_idx(cls, k, 0)] += g;
    words[pht_es_idx(cls, k, 1)] += t;
  }
  w = 1.0;
  k = win->k0;
  while (k < win->khi) {
    k++;
    w = pht_es_up(w, k, win->lam, invk);
    pht_es_word(w, a[2 * k], rn, yr, &g, &t);
    words[pht_es_idx(cls, k, 0)] += g;
    words[pht_es_idx(cls, k, 1)] += t;
  }
}

/* the last row <= K with a non-zero word (-1: none) */
PHT_HD int pht_es_klast(const long long *words, int K) {
  int klast = -1;
  for (int k = 0; k <= K; k++)
    if (words[pht_es_idx(0, k, 0)] | words[pht_es_idx(0, k, 1)] | words[pht_es_idx(1, k, 0)] |
        words[pht_es_idx(1, k, 1)])
      klast = k;
  return klast;
}

/* a step's coefficient: num / den, 0 where the word is 0 or a is not positive */
PHT_HD double pht_es_coef(double word, double den, double a) { return (word != 0.0 && a > 0.0) ? word / den : 0.0; }

/* the six coefficients of step k [czx, czc, cnx, cnc, cex, cac] from rows k and
 * k + 1 of the table ((axn, acn) are not read where k = K) */
PHT_HD void pht_es_coefs(const long long *words, int k, int K, double yscale, double ax, double ac, double axn,
                         double acn, double *c) {
  const double gsc = 1.0 / PHT_ES_PSCALE, tsc = yscale * gsc, k1 = (double)(k + 1);
  c[0] = pht_es_coef((double)words[pht_es_idx(0, k, 1)] * tsc, k1 * ax, ax);
  c[1] = pht_es_coef((double)words[pht_es_idx(1, k, 1)] * tsc, k1 * ac, ac);
  c[2] = (k < K) ? pht_es_coef((double)words[pht_es_idx(0, k + 1, 0)] * gsc, axn, axn) : 0.0;
  c[3] = (k < K) ? pht_es_coef((double)words[pht_es_idx(1, k + 1, 0)] * gsc, acn, acn) : 0.0;
  c[4] = pht_es_coef((double)words[pht_es_idx(0, k, 0)] * gsc, ax, ax);
  c[5] = pht_es_coef((double)words[pht_es_idx(1, k, 0)] * gsc, ac, ac);
}

/* Z[n], N[n n] (N[i + j n]: from i to j, the diagonal 0), E[n], A[n] of one draw
 * (S column-major) from its words, rows 0..K (n <= 32, K <= PHT_LLU_MAXK).
 * Returns the draw's flag word; a flagged draw gives NaN everywhere.  Host
 * only: it keeps the table and the matrices on the stack. */
PHT_HD unsigned pht_es_contract(int n, const double *S, const double *s, const long long *words, int K, double yscale,
                                double *Z, double *N, double *E, double *A) {
  double meta[PHT_LLU_META];
  const unsigned flag = pht_llu_meta(n, S, s, 0.0, meta);
  for (int i = 0; i < n; i++) Z[i] = E[i] = A[i] = flag ? NAN : 0.0;
  for (int i = 0; i < n * n; i++) N[i] = flag ? NAN : 0.0;
  if (flag) return flag;
  const int klast = pht_es_klast(words, K);
  if (klast < 0) return 0;
  double tab[2 * PHT_ES_ROWS], R[32 * 32], Hx[32 * 32], Hc[32 * 32], Hxn[32 * 32], Hcn[32 * 32], f[32], fn[32];
  const double mu = meta[PHT_LLU_M_MU], rinv = 1.0 / mu;
  const int Kt = (klast < K) ? klast + 1 : K;
  pht_llu_table(n, S, s, mu, Kt, tab);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      R[i * n + j] = pht_llu_R(S[i + j * n], rinv, i == j);
      Hx[i * n + j] = (i == 0) ? s[j] : 0.0;
      Hc[i * n + j] = (i == 0) ? 1.0 : 0.0;
    }
  for (int i = 0; i < n; i++) f[i] = (i == 0) ? 1.0 : 0.0;
  for (int k = 0; k <= klast; k++) {
    double c[6];
    pht_es_coefs(words, k, K, yscale, tab[2 * k], tab[2 * k + 1], (k < K) ? tab[2 * k + 2] : 0.0,
                 (k < K) ? tab[2 * k + 3] : 0.0, c);
    for (int i = 0; i < n; i++) {
      A[i] = fma(c[5], f[i], A[i]);
      Z[i] = fma(c[0], Hx[i * n + i], Z[i]);
      Z[i] = fma(c[1], Hc[i * n + i], Z[i]);
      E[i] = fma(c[4], f[i] * s[i], E[i]);
      for (int j = 0; j < n; j++) {
        if (i == j) continue;
        N[i + j * n] = fma(c[2], R[i * n + j] * Hx[i * n + j], N[i + j * n]);
        N[i + j * n] = fma(c[3], R[i * n + j] * Hc[i * n + j], N[i + j * n]);
      }
    }
    if (k == klast) break;
    for (int j = 0; j < n; j++) {
      double v = 0.0;
      for (int l = 0; l < n; l++) v = fma(f[l], R[l * n + j], v);
      fn[j] = v;
    }
    for (int i = 0; i < n; i++)
      for (int j = 0; j < n; j++) {
        double x = 0.0, cc = 0.0;
        for (int l = 0; l < n; l++) {
          x = fma(Hx[i * n + l], R[j * n + l], x);
          cc = fma(Hc[i * n + l], R[j * n + l], cc);
        }
        Hxn[i * n + j] = fma(fn[i], s[j], x);
        Hcn[i * n + j] = fma(fn[i], 1.0, cc);
      }
    for (int i = 0; i < n; i++) f[i] = fn[i];
    for (int i = 0; i < n * n; i++) {
      Hx[i] = Hxn[i];
      Hc[i] = Hcn[i];
    }
  }
  return 0;
}

#endif /* PHT_ESTEP_H */
