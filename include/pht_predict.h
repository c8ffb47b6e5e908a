/*
 * pht_predict.h — specification of the posterior-predictive replicates of a
 * draw: absorption times of PH(e_1, S) simulated forward, and their exact
 * integer reductions.  Shared by the HIP kernel
 * (phasetype_amd/csrc/pht_predict.hip), the host (host_predict.cpp) and the
 * tests' CPU restatement (tests/predict_spec.c).
 *
 * Per draw (pht_pred_build, host): from (S column-major n x n, s) the table of
 * pht_pred_tab_words(n) = n + n n doubles
 *   scale[j]  = 1 / (-S_jj)
 *   cum[j][q], q = 0..n-1: the running sums of the jump probabilities over the
 *             candidates of row j in increasing k, k = j skipped, the exit
 *             last: candidate q is state q + (q >= j) for q < n - 1 and the
 *             exit (state n) for q = n - 1;  Pf(j, k) = S_jk scale_j,
 *             Pf(j, n) = s_j scale_j;  cum[j][q] = cum[j][q - 1] + Pf (from
 *             0.0, sequentially): the additions mhrs_attempt performs per jump.
 *             From the row's LAST candidate of positive probability on the
 *             entries are stored as +inf: the categorical rule below then ends
 *             there whatever u is, which is the overrun rule (DESIGN.md 8
 *             item 2: a rounding overrun takes the last candidate of positive
 *             probability) in table form.  The entries before it are the sums
 *             themselves, and a candidate of zero probability is never taken.
 * Draw flags (non-zero: the draw is skipped, its words stay zero, as a flagged
 * log-likelihood block): PHT_LL_F_NONFINITE a non-finite entry; PHT_LL_F_MU
 * some -S_jj not positive and finite; PHT_PRED_F_RATE a negative off-diagonal
 * or exit rate; PHT_PRED_F_ABSORB absorption is not certain from state 0: a
 * state reachable from state 0 over positive rates cannot reach any state
 * with s_k > 0.
 *
 * Per replicate r of draw d (pht_pred_path): the stream is
 *   pht_stream_init(k0, k1, obs = rep0 + r, tag = PHT_PRED_TAG, sweep = draw0 + d)
 * (PHT_PRED_TAG = 1023 << 22: the MHRS tags are (c + 1) << 22 | att with
 * c + 1 <= 1022, the main streams' 0, the gamma stream's 0x7FFFFFFF on
 * observation numbers from 2^32 - 1 down).  j = 0, t = 0 (pi = e_1), then per
 * jump
 *   more than max_jumps jumps: the replicate is BAD;
 *   t = t + scale[j] * (-pht_log_pos(pht_next_uexp))      (dev_rexp)
 *   t >= horizon: the path stops, y = horizon, counted in nsurv;
 *   u = pht_next_u;  q = the number of cum[j][.] < u  (= the first candidate
 *   with !(cum < u): the sums do not decrease);  j = that candidate's state;
 *   j = n: absorbed, y = t.
 * A recorded y >= 2^20 or not finite is bad as well.  A bad replicate is
 * counted in nbad and nothing else (pointwise NaN).
 *
 * Per-draw reductions, all integers (any grid, batch, replicate split or rank
 * gives the same words): int64 [Hy, Fy, Hq, Fq, ndone, nbad, nsurv, njump],
 * (H, F) = pht_ll_fixed of y and of the one rounded product y * y, njump the
 * jumps of the recorded replicates; ymin / ymax combine by min / max (y >= 0:
 * the order of the 64-bit patterns); with ne edges (strictly increasing,
 * finite, ne <= 1024) counts[ne + 1], the bin of y = the number of edges <= y.
 * No overflow: y < 2^20, so |h| <= 2^20 and 2^40 for the square, |f| <= 2^31;
 * a call takes at most 2^22 replicates per draw, so a call's sums stay below
 * 2^62; sums across calls are the caller's (2^63 at 2 more such calls at the
 * extreme y, far more at any practical one).
 *
 * Every operation is explicit; every unit that includes this is compiled with
 * -ffp-contract=off; the log is include/pht_detmath.h's.  A GPU lane and the
 * CPU restatement give the same bits.
 */
#ifndef PHT_PREDICT_H
#define PHT_PREDICT_H

#include "pht_loglik_unif.h" /* pht_ll_fixed, PHT_LL_F_NONFINITE, PHT_LL_F_MU */
#include "pht_philox.h"

#define PHT_PRED_F_RATE 16u   /* a negative off-diagonal or exit rate */
#define PHT_PRED_F_ABSORB 32u /* absorption is not certain from state 0 */

#define PHT_PRED_TAG 0xFFC00000u    /* 1023 << 22: no sampler's stream tag */
#define PHT_PRED_MAXN 32
#define PHT_PRED_YMAX 1048576.0     /* 2^20: a recorded y at or above is bad */
#define PHT_PRED_MAXREP (1 << 22)   /* replicates per draw and call */
#define PHT_PRED_MAXEDGES 1024
#define PHT_PRED_MAXJUMPS (1 << 20) /* = kMaxJumps */

/* per-draw int64 words */
#define PHT_PRED_WORDS 8
#define PHT_PRED_W_HY 0
#define PHT_PRED_W_FY 1
#define PHT_PRED_W_HQ 2
#define PHT_PRED_W_FQ 3
#define PHT_PRED_W_NDONE 4
#define PHT_PRED_W_NBAD 5
#define PHT_PRED_W_NSURV 6
#define PHT_PRED_W_NJUMP 7

/* outcome of a replicate */
#define PHT_PRED_BAD 1
#define PHT_PRED_SURV 2

PHT_HD int pht_pred_tab_words(int n) { return n + n * n; }

/* the flag word of a draw (0 = usable) */
PHT_HD unsigned pht_pred_flags(int n, const double *S, const double *s) {
  unsigned flag = 0;
  for (int k = 0; k < n * n; k++)
    if (!(fabs(S[k]) < INFINITY)) flag |= PHT_LL_F_NONFINITE;
  for (int k = 0; k < n; k++)
    if (!(fabs(s[k]) < INFINITY)) flag |= PHT_LL_F_NONFINITE;
  if (flag) return flag;
  for (int j = 0; j < n; j++) {
    const double v = -S[j + j * n];
    if (!((v > 0.0) && (v < INFINITY))) flag |= PHT_LL_F_MU;
    if (s[j] < 0.0) flag |= PHT_PRED_F_RATE;
    for (int k = 0; k < n; k++)
      if (k != j && S[j + k * n] < 0.0) flag |= PHT_PRED_F_RATE;
  }
  if (flag) return flag;
  /* reach[j]: reachable from state 0; out[j]: reaches a state with s > 0;
   * both over the positive rates, to their fixed points (n <= 32 rounds) */
  int reach[PHT_PRED_MAXN], out[PHT_PRED_MAXN];
  for (int j = 0; j < n; j++) {
    reach[j] = (j == 0);
    out[j] = (s[j] > 0.0);
  }
  for (int round = 0; round < n; round++)
    for (int j = 0; j < n; j++)
      for (int k = 0; k < n; k++)
        if (k != j && S[j + k * n] > 0.0) {
          if (reach[j]) reach[k] = 1;
          if (out[k]) out[j] = 1;
        }
  for (int j = 0; j < n; j++)
    if (reach[j] && !out[j]) flag |= PHT_PRED_F_ABSORB;
  return flag;
}

/* the state of candidate q of row j (n = the exit) */
PHT_HD int pht_pred_state(int n, int j, int q) { return (q == n - 1) ? n : q + (q >= j ? 1 : 0); }

/* the table of a usable draw: tab[j] = scale[j], tab[n + j n + q] = cum[j][q] */
PHT_HD void pht_pred_table(int n, const double *S, const double *s, double *tab) {
  for (int j = 0; j < n; j++) {
    const double scale = 1.0 / -S[j + j * n];
    double *cum = tab + n + j * n;
    double sofar = 0.0;
    int last = 0;
    tab[j] = scale;
    for (int q = 0; q < n; q++) {
      const int k = pht_pred_state(n, j, q);
      const double pf = ((k < n) ? S[j + k * n] : s[j]) * scale;
      sofar = sofar + pf;
      cum[q] = sofar;
      if (pf > 0.0) last = q;
    }
    for (int q = last; q < n; q++) cum[q] = INFINITY;
  }
}

/* the categorical jump from a row's running sums */
PHT_HD int pht_pred_select(const double *cum, int n, double u) {
  int q = 0;
  for (int i = 0; i < n - 1; i++) q += (cum[i] < u) ? 1 : 0; /* (cum[n - 1] = +inf never counts) */
  return q;
}

/* the sojourn and the jump of one step from state j at time *t: returns the
 * next state (n: absorbed), or -1 when the sojourn reached the horizon.
 * cum[j * ld + q]: the table's rows at a leading dimension ld >= n (n in the
 * table itself; the kernel's LDS copy pads it) */
PHT_HD int pht_pred_step(int n, const double *scale, const double *cum, int ld, int j, double horizon, pht_stream *r,
                         double *t) {
  *t = *t + scale[j] * -pht_log_pos(pht_next_uexp(r));
  if (*t >= horizon) return -1;
  const double u = pht_next_u(r);
  return pht_pred_state(n, j, pht_pred_select(cum + j * ld, n, u));
}

/* the recorded value of a finished path: horizon for a stopped one; the
 * outcome gains PHT_PRED_BAD for y >= 2^20 or not finite */
PHT_HD double pht_pred_record(double t, double horizon, int *outcome) {
  const double y = (*outcome & PHT_PRED_SURV) ? horizon : t;
  if (!(y < PHT_PRED_YMAX)) *outcome |= PHT_PRED_BAD;
  return y;
}

/* one replicate, sequentially: y (NaN when bad), *njump, *outcome */
PHT_HD double pht_pred_path(int n, const double *tab, uint32_t k0, uint32_t k1, uint32_t rep, uint32_t draw,
                            double horizon, int max_jumps, int *njump, int *outcome) {
  pht_stream r;
  pht_stream_init(&r, k0, k1, rep, PHT_PRED_TAG, draw);
  int j = 0, nj = 0, oc = 0;
  double t = 0.0;
  for (;;) {
    if (nj >= max_jumps) {
      oc = PHT_PRED_BAD;
      break;
    }
    nj++;
    j = pht_pred_step(n, tab, tab + n, n, j, horizon, &r, &t);
    if (j < 0) oc = PHT_PRED_SURV;
    if (j < 0 || j == n) break;
  }
  *njump = nj;
  const double y = (oc & PHT_PRED_BAD) ? NAN : pht_pred_record(t, horizon, &oc);
  *outcome = oc;
  return (oc & PHT_PRED_BAD) ? NAN : y;
}

/* the bin of y: the number of edges <= y (binary search; ne >= 0) */
PHT_HD int pht_pred_bin(const double *edges, int ne, double y) {
  int lo = 0, hi = ne; /* edges[lo - 1] <= y < edges[hi] */
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (edges[mid] <= y) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

#endif /* PHT_PREDICT_H */
