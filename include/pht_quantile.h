/*
 * pht_quantile.h — specification of the quantile function of a phase-type
 * draw and of its residual life: the "q" of d / p / q / r.  For one draw
 * (S, s) with pi = e_1, a probability p and a conditioning time t0 >= 0, the
 * t >= t0 with
 *   log Fbar(t) = L,   L = log(1 - p) + log Fbar(t0),
 * i.e. P(T <= t | T > t0) = p; the result is t - t0 for t0 > 0 (a residual
 * life) and t for t0 = 0.  No reference counterpart.  Shared by the HIP kernel
 * (phasetype_amd/csrc/pht_quantile.hip), the host (host_quantile.cpp) and the
 * tests' CPU restatement (tests/quantile_spec.c).
 *
 * Function values.  Only include/pht_loglik_unif.h's pht_llu_eval, unchanged,
 * on the draw's table (ax_k, ac_k): lS(t) = log Fbar(t) (cens = 1), lf(t) =
 * log f(t) (cens = 0), hazard(t) = pht_exp(lf - lS).  Since ax_k = mu (ac_k -
 * ac_{k+1}), lf is the exact derivative of the same series: Newton's step on
 * h(t) = lS(t) - L is t + h / hazard.  log(1 - p) is pht_psis.h's compensated
 * pht_psis_log1p(-p); t0 = 0 contributes exactly 0 without an evaluation, and
 * lS(t0) is evaluated once per draw for t0 > 0.  The evaluation count of a
 * root does not include the draw's two evaluations at t0.
 *
 * Table and horizon per draw (pht_q_meta).  mu = max_i -S_ii as in
 * pht_llu_meta; the horizon is t_hi = min(tmax, PHT_Q_LAMBDA / mu) and the
 * draw's meta words are pht_llu_meta(n, S, s, t_hi, .), so the table has
 * K = pht_llu_K(mu, t_hi) rows.  PHT_Q_LAMBDA = 1400: mu t_hi <= 1400 (1 +
 * 2^-52), and ceil(1400 + 14 sqrt(1400) + 64) = ceil(1987.84) = 1988 <=
 * PHT_LLU_MAXK = 2047 with 59 rows to spare (the largest Lambda of that form
 * is 1456; the room covers the rounding of mu t_hi and keeps the tables of four
 * draws, 1 / k and the math tables within 160 KB of LDS).  tmax = +inf means
 * "as far as the table cap allows".  A survival function still above 1 - p at
 * 1400 mean sojourn times of the fastest state is reported BEYOND, not found.
 *
 * Iteration (pht_q_root), every order fixed.  Invariant: a bracket [a, b],
 * a = t0 and b = t_hi at the start, with h(a) >= 0 from a good evaluation
 * (h(t0) = -log1p(-p) >= 0 needs none) and b either a good evaluation with
 * h(b) <= 0 or an evaluation that pht_llu_eval reported bad (bbad; in
 * practice Fbar(b) below the evaluator's floor 2^-900, the usual state of
 * b = t_hi for a light-tailed draw: n = 1 has Fbar(t_hi) = e^-1400).  A bad
 * point is never used as a function value: it only serves as a provisional
 * upper end, and a root is returned only from a bracket whose two ends are
 * good evaluations.  If the search ends with b still bad the result is NaN
 * with PHT_Q_F_EVAL: never a silent value.
 *   1. lS(b), b = t_hi.  Good and h(b) > 0: +inf, PHT_Q_F_BEYOND.
 *   2. The first Newton step starts from x = a = t0 with hazard(t0), which
 *      like lS(t0) is evaluated once per draw (pht_q_start), not per root
 *      (for a small p the step is -log1p(-p) / hazard(t0), nearly the root;
 *      with a structural zero s_1 = 0 and t0 = 0 there is no density at 0
 *      and the first step is forced).
 *   3. Until the stop rule holds: each end keeps its h and its hazard (0
 *      where it has none: b bad, lf bad, or a hazard not positive and
 *      finite; lf(t_hi) is not evaluated).  From the end x with a usable
 *      hazard and the smaller |h| (a on a tie), cand = x + h(x) / hazard(x),
 *      then pushed on by tau = 2^-46 cand in its direction of travel (cand +
 *      tau from a, cand - tau from b): a converged Newton sequence approaches
 *      from one side and would never move the other end; the push lands just
 *      beyond the root, so two such steps close the bracket to about 2 tau.
 *      The step is TAKEN if the pushed candidate lies strictly inside (a, b)
 *      and fewer than PHT_Q_RUN = 3 Newton steps were taken since the bracket
 *      last halved; otherwise it is FORCED: t = a + (b - a) / 2 (the next
 *      double above a where that is not strictly inside).  "Halved": w_ref
 *      is the width b - a at the last forced step or checkpoint; whenever
 *      b - a <= w_ref / 2 after a step, w_ref = b - a and the count restarts
 *      (a checkpoint).  Evaluate lS(t): bad: b = t, bbad = 1;  h > 0: a = t;
 *      h < 0: b = t, bbad = 0;  h = 0: a = b = t.  For a good t, lf(t) gives
 *      that end's hazard.
 *   4. Stop: b - a <= 2^-44 b, or a and b adjacent doubles (or equal).
 *      t^ = a + (b - a) / 2, kept inside [a, b].
 * Cap.  Every PHT_Q_RUN + 1 consecutive steps contain a checkpoint or a
 * forced step, and a forced step leaves at most half the width plus one
 * rounding.  Two finite non-negative doubles are at most 2^1024 apart and at
 * least 2^-1074, so after 2099 halvings a and b are adjacent; with slack for
 * the roundings, PHT_Q_MAXIT = 4 * 2200 = 8800 steps always suffice.  Reaching
 * it sets PHT_Q_F_CAP and gives NaN (no input of the tests comes near: the
 * largest count observed is recorded in DESIGN.md 5h).
 *
 * Outputs per (draw, p): t^ (as a residual life for t0 > 0), the final a and
 * b (absolute times), the number of pht_llu_eval calls, and a flag word.
 *   p = 0: t^ = t0 (result 0), a = b = t0.  p = 1: +inf, a = b = +inf.
 *   p NaN or outside [0, 1]: NaN, PHT_Q_F_P.  t0 not finite and
 *   non-negative: NaN, PHT_Q_F_T0.  t0 >= t_hi, or h(t_hi) > 0: +inf,
 *   PHT_Q_F_BEYOND, a = max(t0, t_hi), b = +inf (a generator that never
 *   absorbs ends here).  lS(t0) bad, or no good upper end: NaN,
 *   PHT_Q_F_EVAL.  A draw flagged by pht_llu_meta: NaN for all its p, never
 *   evaluated, PHT_Q_F_DRAW (the draw's flag word is returned as well).
 *
 * Error bound.  With eps(t) = 2^-53 (n + 9) (k_hi(t) + 1) + 2^-56 the
 * evaluator's bound and Fbar_true decreasing, log Fbar_true(t^) lies between
 * the true values at b and a, which differ by at most hazard_max (b - a),
 * hazard_max = max_j s_j (the hazard is a convex combination of the s_j;
 * abar_x of the meta words), and the computed lS(a) >= L >= lS(b):
 *   |log Fbar_true(t^) - L_true| <= eps(a) + eps(b) + eps(t0)
 *                                   + hazard_max (b - a) + dL,
 *   dL = 2^-50 |log1p(-p)| + 2^-53 |L|
 * (pht_log is below 1 ulp, the compensated quotient adds three roundings;
 * the sum L one; eps(t0) = 0 for t0 = 0).  In t the error is that bound
 * divided by the hazard at the root.  Small p: log(1 - p) ~ -p, so the
 * RELATIVE error in p is the bound divided by p.  At n = 10 and k_hi about
 * 100 the bound is about 5e-13, so p >= 5e-7 keeps it below 1e-6; at the
 * worst (n = 32, k_hi = 2047, t0 > 0) the bound is 3e-11 and the floor
 * p >= 3e-5.  Probabilities below the floor are still bracketed and
 * certified, with the relative error bound / p; a lower-tail series is out
 * of scope.
 *
 * Every operation is explicit; every unit that includes this is compiled with
 * -ffp-contract=off; exp and log are include/pht_detmath.h's; divisions are
 * IEEE.  A GPU lane and the CPU restatement give the same bits.
 */
#ifndef PHT_QUANTILE_H
#define PHT_QUANTILE_H

#include "pht_loglik_unif.h"
#include "pht_psis.h" /* pht_psis_log1p */

#define PHT_Q_LAMBDA 1400.0 /* mu t_hi at most: K = 1988 <= PHT_LLU_MAXK */
#define PHT_Q_RUN 3         /* Newton steps without a halving before a forced step */
#define PHT_Q_MAXIT 8800    /* steps: (PHT_Q_RUN + 1) * 2200 halvings */
#define PHT_Q_RTOL 0x1p-44  /* stop: b - a <= PHT_Q_RTOL b */
#define PHT_Q_PUSH 0x1p-46  /* a Newton candidate is pushed on by this fraction */

#define PHT_Q_F_P 1u       /* p NaN or outside [0, 1] */
#define PHT_Q_F_T0 2u      /* t0 not finite and non-negative */
#define PHT_Q_F_BEYOND 4u  /* the root lies beyond the horizon / the table cap */
#define PHT_Q_F_EVAL 8u    /* no bracket of good evaluations (pht_llu_eval bad) */
#define PHT_Q_F_CAP 16u    /* PHT_Q_MAXIT reached */
#define PHT_Q_F_DRAW 32u   /* the draw is flagged (pht_llu_meta) */

typedef struct {
  double t, a, b; /* the result; the final bracket (absolute times) */
  int nev;        /* pht_llu_eval calls of this root */
  unsigned flags;
} pht_q_out_t;

/* the horizon of a usable draw */
PHT_HD double pht_q_thi(double mu, double tmax) {
  double th = PHT_Q_LAMBDA / mu;
  if (!(th < INFINITY)) th = 0x1.fffffffffffffp+1023; /* a subnormal mu */
  return (tmax < th) ? tmax : th;
}

/* one draw's meta words (pht_llu_meta's, K for the draw's own horizon) and
 * *thi (0 for a flagged draw); returns the flag word */
PHT_HD unsigned pht_q_meta(int n, const double *S, const double *s, double tmax, double *meta, double *thi) {
  unsigned flag = pht_llu_meta(n, S, s, 0.0, meta);
  *thi = 0.0;
  if (flag) return flag;
  *thi = pht_q_thi(meta[PHT_LLU_M_MU], tmax);
  return pht_llu_meta(n, S, s, *thi, meta);
}

/* t0 usable: finite and non-negative */
PHT_HD int pht_q_t0_ok(double t0) { return (t0 >= 0.0) && (t0 < INFINITY); }

/* the start of a usable draw's searches, once per draw: lS(t0) (0 without an
 * evaluation for t0 = 0) and hazard(t0) (0 where lf(t0) is bad or the hazard
 * is not positive and finite: the first step is then forced); nothing is
 * evaluated where no root will be searched (t0 unusable or at or beyond t_hi) */
PHT_HD double pht_q_start(const double *tab, const double *invk, int K, double mu, double abar_x, double thi, double t0,
                          int *bad0, double *hz0) {
  *bad0 = 0;
  *hz0 = 0.0;
  if (!pht_q_t0_ok(t0) || !(t0 < thi)) return 0.0;
  int khi, badf;
  double ls0 = 0.0;
  if (t0 > 0.0) ls0 = pht_llu_eval(tab, invk, K, mu, abar_x, t0, 1, bad0, &khi);
  if (*bad0) return 0.0;
  const double lf = pht_llu_eval(tab, invk, K, mu, abar_x, t0, 0, &badf, &khi);
  const double hz = badf ? 0.0 : pht_exp(lf - ls0);
  *hz0 = ((hz > 0.0) && (hz < INFINITY)) ? hz : 0.0;
  return ls0;
}

/* a and b adjacent doubles or equal (0 <= a <= b finite) */
PHT_HD int pht_q_adjacent(double a, double b) { return pht_d2u(b) - pht_d2u(a) <= 1ull; }

PHT_HD int pht_q_stop(double a, double b) { return (b - a <= PHT_Q_RTOL * b) || pht_q_adjacent(a, b); }

/* the forced step: the midpoint, strictly inside (a, b) for non-adjacent ends */
PHT_HD double pht_q_mid(double a, double b) {
  const double t = a + 0.5 * (b - a);
  return (t > a && t < b) ? t : pht_u2d(pht_d2u(a) + 1ull);
}

PHT_HD void pht_q_set(pht_q_out_t *o, double t, double a, double b, int nev, unsigned flags) {
  o->t = t;
  o->a = a;
  o->b = b;
  o->nev = nev;
  o->flags = flags;
}

/* one root of a usable draw: the table, invk[k] = 1 / k, the meta words' K,
 * mu, abar_x, the horizon, t0 with lS(t0), its bad flag and hazard(t0)
 * (pht_q_start), p */
PHT_HD void pht_q_root(const double *tab, const double *invk, int K, double mu, double abar_x, double thi, double t0,
                       double ls0, int bad0, double hz0, double p, pht_q_out_t *o) {
  if (!(p >= 0.0 && p <= 1.0)) {
    pht_q_set(o, NAN, NAN, NAN, 0, PHT_Q_F_P);
    return;
  }
  if (!pht_q_t0_ok(t0)) {
    pht_q_set(o, NAN, NAN, NAN, 0, PHT_Q_F_T0);
    return;
  }
  if (p == 0.0) {
    pht_q_set(o, 0.0, t0, t0, 0, 0u);
    return;
  }
  if (p == 1.0) {
    pht_q_set(o, INFINITY, INFINITY, INFINITY, 0, 0u);
    return;
  }
  if (!(t0 < thi)) {
    pht_q_set(o, INFINITY, t0, INFINITY, 0, PHT_Q_F_BEYOND);
    return;
  }
  if (bad0) {
    pht_q_set(o, NAN, NAN, NAN, 0, PHT_Q_F_EVAL);
    return;
  }
  const double L = pht_psis_log1p(-p) + ls0;
  double a = t0, b = thi;
  int nev = 0, bad, khi, bbad;
  /* 1. the upper end */
  double l = pht_llu_eval(tab, invk, K, mu, abar_x, b, 1, &bad, &khi);
  nev++;
  bbad = bad;
  if (!bad && l - L > 0.0) {
    pht_q_set(o, INFINITY, thi, INFINITY, nev, PHT_Q_F_BEYOND);
    return;
  }
  /* 2. the ends' function values and hazards (0: no usable hazard there) */
  double ha = ls0 - L, hza = hz0, hb = bad ? 0.0 : l - L, hzb = 0.0;
  /* 3. the steps */
  double wref = b - a;
  int run = 0, it = 0;
  while (!pht_q_stop(a, b)) {
    if (it >= PHT_Q_MAXIT) {
      pht_q_set(o, NAN, a, b, nev, PHT_Q_F_CAP);
      return;
    }
    it++;
    double t = 0.0;
    int newton = 0;
    if ((hza > 0.0 || hzb > 0.0) && run < PHT_Q_RUN) {
      const int useb = (hzb > 0.0) && (!(hza > 0.0) || -hb < ha);
      const double c = useb ? b + hb / hzb : a + ha / hza;
      t = useb ? c - PHT_Q_PUSH * c : c + PHT_Q_PUSH * c;
      newton = (t > a) && (t < b);
    }
    if (!newton) t = pht_q_mid(a, b);
    l = pht_llu_eval(tab, invk, K, mu, abar_x, t, 1, &bad, &khi);
    nev++;
    if (bad) {
      b = t;
      bbad = 1;
      hzb = 0.0;
    } else {
      const double h = l - L;
      int badf;
      const double lf = pht_llu_eval(tab, invk, K, mu, abar_x, t, 0, &badf, &khi);
      nev++;
      double hz = badf ? 0.0 : pht_exp(lf - l);
      hz = ((hz > 0.0) && (hz < INFINITY)) ? hz : 0.0;
      if (h >= 0.0) {
        a = t;
        ha = h;
        hza = hz;
      }
      if (h <= 0.0) {
        b = t;
        hb = h;
        hzb = hz;
        bbad = 0;
      }
    }
    const double wd = b - a;
    if (newton) run++;
    if (!newton || wd <= 0.5 * wref) {
      wref = wd;
      run = 0;
    }
  }
  if (bbad) {
    pht_q_set(o, NAN, a, b, nev, PHT_Q_F_EVAL);
    return;
  }
  double th = a + 0.5 * (b - a);
  th = (th < a) ? a : ((th > b) ? b : th);
  pht_q_set(o, (t0 > 0.0) ? th - t0 : th, a, b, nev, 0u);
}

/* what a flagged draw gives for every p */
PHT_HD void pht_q_flagged(pht_q_out_t *o) { pht_q_set(o, NAN, NAN, NAN, 0, PHT_Q_F_DRAW); }

/* The whole function for one draw on the host (no device): np roots of
 * (S column-major n x n, s), n <= 32, into t, lo, hi, nev, flags (each np; any
 * may be null).  tab: room for 2 (PHT_LLU_MAXK + 1) doubles, invk: for
 * PHT_LLU_MAXK + 1.  Returns the draw's flag word. */
PHT_HD unsigned pht_q_draw(int n, const double *S, const double *s, int np, const double *probs, double t0,
                           double tmax, double *tab, double *invk, double *t, double *lo, double *hi, int *nev,
                           unsigned *flags) {
  double meta[PHT_LLU_META], thi;
  const unsigned flag = pht_q_meta(n, S, s, tmax, meta, &thi);
  const int K = (int)meta[PHT_LLU_M_K];
  const double mu = meta[PHT_LLU_M_MU], abar = meta[PHT_LLU_M_ABAR];
  double ls0 = 0.0, hz0 = 0.0;
  int bad0 = 0;
  if (!flag) {
    pht_llu_table(n, S, s, mu, K, tab);
    for (int k = 0; k <= K; k++) invk[k] = k ? 1.0 / (double)k : 0.0;
    ls0 = pht_q_start(tab, invk, K, mu, abar, thi, t0, &bad0, &hz0);
  }
  for (int i = 0; i < np; i++) {
    pht_q_out_t o;
    if (flag)
      pht_q_flagged(&o);
    else
      pht_q_root(tab, invk, K, mu, abar, thi, t0, ls0, bad0, hz0, probs[i], &o);
    if (t) t[i] = o.t;
    if (lo) lo[i] = o.a;
    if (hi) hi[i] = o.b;
    if (nev) nev[i] = o.nev;
    if (flags) flags[i] = o.flags;
  }
  return flag;
}

#endif /* PHT_QUANTILE_H */
