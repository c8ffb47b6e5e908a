/*
 * pht_replace.h — specification of the age-replacement policy of a phase-type
 * draw: a unit is replaced at failure (cost cf) or preventively at age tau
 * (cost cp < cf), whichever comes first.  For one draw (S, s) with pi = e_1 the
 * long-run cost rate is
 *   g(tau) = (cp + (cf - cp) F(tau)) / M(tau),   M(tau) = int_0^tau Fbar(u) du,
 *   g(inf) = cf / m,                             m = E[T],
 * and the specification gives the curve (lS, lf, M) on a grid of ages and, per
 * cost pair, the optimal age tau* with its cost rate.  No reference
 * counterpart.  Shared by the HIP kernels (phasetype_amd/csrc/pht_replace.hip),
 * the host (host_replace.cpp) and the tests' CPU restatement
 * (tests/replace_spec.c).
 *
 * Inputs of a call: draws (S, s), n <= 32; G ages, 1 <= G <= PHT_RP_MAXG,
 * finite, > 0, strictly increasing (pht_rp_ages_ok); P cost pairs, 1 <= P <=
 * PHT_RP_MAXP, each usable when 0 < cp < cf < inf (pht_rp_cost_ok).
 *
 * Per draw (pht_rp_meta).  The meta words and the horizon are pht_q_meta's
 * with tmax = the last age: mu t_hi <= 1400 and K <= 1988 rows.  m is the first
 * entry of pht_cd_mean's vector; its PHT_CD_F_TRAP joins the draw's flag word,
 * and a flagged draw is never evaluated (PHT_RP_A_DRAW at every age,
 * PHT_RP_F_DRAW for every pair, every value NaN).  The table (ax_k, ac_k) is
 * pht_llu_table's, unchanged.  The restricted mean needs a third column, the
 * prefix sums of the survival column (pht_rp_cc), sequentially:
 *   cc_0 = 0,  cc_{i+1} = cc_i + ac_i,  i = 0 .. K - 1     (K + 1 entries).
 * Since int_0^tau e^{-mu u} (mu u)^k / k! du = P(Pois(lam) >= k + 1) / mu,
 *   M(tau) = (1 / mu) sum_i Pois(i; lam) cc_i,   lam = mu tau:
 * every term is non-negative, M -> tau as tau -> 0 without cancellation, and
 * cc is non-decreasing and bounded by mu m.
 *
 * pht_rp_rmean is pht_llu_eval's mode-relative window on the cc column:
 * k0 = min(floor(lam), K), w_k0 = 1, num = cc[k0], den = 1; downward
 * w <- w (k / lam), k <- k - 1, upward k <- k + 1, w <- w (lam invk[k]); in
 * both num = fma(w, cc[k], num), den = den + w.  Each direction stops BEFORE
 * the term for which  w < 2^-60  and  w u < 2^-60 num  hold, u a bound of every
 * cc still to come: downward u = cc[k] (cc is non-decreasing), upward
 * u = cc[K], the column's last entry (not abar ac_k: cc does not decay).  An
 * upward sweep at k = K with the rule unmet is BAD (the table is too short),
 * and so are !(lam > 0) and an M that is not positive and finite.
 *   M = (num / den) / mu.
 *
 * Curve, per (draw, age) (pht_rp_curve): an age beyond the draw's horizon
 * (tau > t_hi) is PHT_RP_A_BEYOND; otherwise lS = pht_llu_eval(cens = 1),
 * lf = pht_llu_eval(cens = 0), M = pht_rp_rmean, and any bad one of the three
 * gives PHT_RP_A_EVAL.  A flagged age has lS = lf = M = NaN, is counted by the
 * caller and never enters an argmin.  From the three values:
 *   F = pht_fc_q(lS),  h = pht_exp(lf - lS),
 *   g = (cp + (cf - cp) F) / M,
 *   D = (h M - F) - c0,  c0 = cp / (cf - cp);   sign g'(tau) = sign D(tau),
 * D(0+) < 0 always, and g(tau*) = (cf - cp) h(tau*) at an interior optimum.
 *
 * Policy, per (draw, cost pair) (pht_rp_policy), every order fixed:
 *   1. g at every good age; j = the first index of the smallest g (a g that
 *      is NaN never wins); g_inf = cf / m.  No good age: NaN, PHT_RP_F_NOAGE.
 *   2. D(tau_j) from the curve's values.  D >= 0: the bracket is
 *      [tau_{j-1}, tau_j], tau_{-1} := 0 where D < 0 needs no evaluation.
 *      D < 0: if no good age lies above j the result is tau_j with
 *      PHT_RP_F_EDGE (the cost rate still falls where the grid ends);
 *      otherwise the bracket is [tau_j, tau_{j+1}].  The far end must be a
 *      good age whose D has the opposite sign (D < 0 at a lower, D >= 0 at an
 *      upper end); if not, the result is tau_j with PHT_RP_F_UNREFINED.  For
 *      EDGE and UNREFINED g = g_j, lo = hi = tau_j, nev = 0.
 *   3. Refinement keeps D(a) < 0 <= D(b).  A multisection step evaluates D at
 *      the 64 points  t_i = a + (i (b - a)) / 65,  i = 1 .. 64  (pht_rp_point;
 *      t_0 = a), provided a < t_1 < ... < t_64 < b (pht_rp_inside, "strictly
 *      inside").  The first i with D(t_i) >= 0 gives b = t_i, a = t_{i-1}
 *      (D = 0 counts as >= 0: the tie goes to the upper end); none gives
 *      a = t_64.  It stops when b - a <= 2^-40 b (PHT_RP_RTOL) or a and b are
 *      adjacent doubles.  When the points are not strictly inside, the steps
 *      are midpoints t = pht_q_mid(a, b) with the same rule until the stop
 *      holds.  A bad evaluation at any point ends the search: NaN,
 *      PHT_RP_F_EVAL.  Cap: a multisection step leaves at most 1 / 65 of the
 *      width plus roundings, and two finite non-negative doubles are at most
 *      2^2098 apart in ratio: 349 such steps, then at most 7 midpoint steps
 *      (fewer than 130 doubles between the ends); PHT_RP_MAXSTEP = 400 steps of
 *      either kind, reaching it gives NaN with PHT_RP_F_CAP.
 *   4. t^ = a + (b - a) / 2 kept inside [a, b]; g at t^ from one more
 *      evaluation (bad: NaN, PHT_RP_F_EVAL); lo = a, hi = b; nev = the points
 *      at which the three series were evaluated (64 a multisection step, 1 a
 *      midpoint step, 1 for t^).
 *   5. If g_inf <= the g found (refined, EDGE or UNREFINED): t = +inf,
 *      g = g_inf, PHT_RP_F_NEVER; lo, hi, j keep the finite candidate.
 *   An unusable pair: NaN, j = -1, PHT_RP_F_COST.
 * The GPU puts the 64 points of a step into the 64 lanes of a wavefront and
 * finds the sign change by ballot; the host walks them in a loop: the same
 * points, the same values, the same choice.
 *
 * Error bounds.  eps(k) = 2^-53 (n + 9) (k + 1) + 2^-56 is pht_llu_eval's
 * bound with k the upper end of the window (for M the window of pht_rp_rmean).
 *   |M^ - M| <= PHT_RP_M_R eps(k_hi) M,
 *   |D^ - D| <= PHT_RP_D_R eps(k_hi) (h M + F + c0),
 * k_hi the largest of the three windows.  The constants are measured against
 * mpmath (60 digits) over bd3, bd10, erlang6, acyclic6, reversible6,
 * neareq12, stiff6, hypoexp6, coxian_shared6 and gapped6: M at
 * mu tau in {1e-9, 1e-3, 1, 30, 1000}, D at the seven ages m (0.05 .. 3.2) and
 * the returned brackets; with a margin of 4 (the largest ratios observed are
 * recorded in DESIGN.md 5l; tests/test_replace.py recomputes them).
 *
 * Every operation is explicit; every unit that includes this is compiled with
 * -ffp-contract=off; exp and log are include/pht_detmath.h's; divisions are
 * IEEE.  A GPU lane and the CPU restatement give the same bits.
 */
#ifndef PHT_REPLACE_H
#define PHT_REPLACE_H

#include "pht_condition.h"
#include "pht_forecast.h"
#include "pht_quantile.h"

#define PHT_RP_MAXG 1024 /* ages of a call */
#define PHT_RP_MAXP 16   /* cost pairs of a call */
#define PHT_RP_NPT 64    /* points of a multisection step: the lanes of a wavefront */
#define PHT_RP_RTOL 0x1p-40 /* stop: b - a <= PHT_RP_RTOL b */
#define PHT_RP_MAXSTEP 400  /* steps of a refinement, of either kind */

#define PHT_RP_M_R 0.185 /* measured bound of M in units of eps(k_hi) M, margin 4 */
#define PHT_RP_D_R 0.469 /* measured bound of D in units of eps(k_hi) (h M + F + c0), margin 4 */

/* age flags */
#define PHT_RP_A_BEYOND 1u /* tau beyond the draw's horizon (mu tau > 1400) */
#define PHT_RP_A_EVAL 2u   /* a bad evaluation of lS, lf or M */
#define PHT_RP_A_DRAW 4u   /* the draw is flagged */

/* policy flags */
#define PHT_RP_F_COST 1u      /* not 0 < cp < cf < inf */
#define PHT_RP_F_DRAW 2u      /* the draw is flagged (pht_q_meta) or trapped (pht_cd_mean) */
#define PHT_RP_F_NOAGE 4u     /* no good age */
#define PHT_RP_F_UNREFINED 8u /* no far end of the opposite sign: the grid's argmin */
#define PHT_RP_F_EDGE 16u     /* the cost rate still falls at the last good age */
#define PHT_RP_F_EVAL 32u     /* a bad evaluation inside the bracket */
#define PHT_RP_F_NEVER 64u    /* g_inf <= the g found: never replace preventively */
#define PHT_RP_F_CAP 128u     /* PHT_RP_MAXSTEP reached */

typedef struct {
  double t, g, lo, hi;
  int j, nev;
  unsigned flags;
} pht_rp_out_t;

/* doubles of pht_rp_draw's workspace: tab, cc, invk and the curve (lS, lf, M) */
#define PHT_RP_WORK(G) ((size_t)4 * (PHT_LLU_MAXK + 1) + (size_t)3 * (size_t)(G))

/* 1 <= G <= 1024, every age finite and > 0, strictly increasing */
PHT_HD int pht_rp_ages_ok(int G, const double *ages) {
  if (G < 1 || G > PHT_RP_MAXG) return 0;
  for (int i = 0; i < G; i++) {
    if (!(ages[i] > 0.0) || !(ages[i] < INFINITY)) return 0;
    if (i && !(ages[i] > ages[i - 1])) return 0;
  }
  return 1;
}

PHT_HD int pht_rp_cost_ok(double cp, double cf) { return (cp > 0.0) && (cf > cp) && (cf < INFINITY); }

/* eps(k) of the error bounds */
PHT_HD double pht_rp_eps(int n, int khi) { return 0x1p-53 * ((double)(n + 9) * (double)(khi + 1)) + 0x1p-56; }
PHT_HD double pht_rp_M_bound(int n, int khi, double M) { return (PHT_RP_M_R * pht_rp_eps(n, khi)) * M; }
/* hM = h M, F and c0 of the truth */
PHT_HD double pht_rp_D_bound(int n, int khi, double hM, double F, double c0) {
  return (PHT_RP_D_R * pht_rp_eps(n, khi)) * (hM + F + c0);
}

/* one draw's meta words (pht_q_meta's for tmax = the last age), its horizon
 * and m = E[T]; returns the flag word, PHT_CD_F_TRAP included: the words of a
 * flagged draw are zero but for the flag, *thi = 0 and *m = NaN */
PHT_HD unsigned pht_rp_meta(int n, const double *S, const double *s, double tmax, double *meta, double *thi, double *m) {
  unsigned flag = pht_q_meta(n, S, s, tmax, meta, thi);
  *m = NAN;
  if (flag) return flag;
  double mv[32];
  flag = pht_cd_mean(n, S, s, mv);
  if (flag) {
    meta[PHT_LLU_M_FLAG] = pht_u2d((uint64_t)flag);
    meta[PHT_LLU_M_MU] = meta[PHT_LLU_M_ABAR] = meta[PHT_LLU_M_K] = 0.0;
    *thi = 0.0;
    return flag;
  }
  *m = mv[0];
  return 0u;
}

/* cc[0 .. K] from the table's survival column, sequentially */
PHT_HD void pht_rp_cc(const double *tab, int K, double *cc) {
  double v = 0.0;
  cc[0] = v;
  for (int i = 0; i < K; i++) {
    v = v + tab[2 * i + 1];
    cc[i + 1] = v;
  }
}

PHT_HD int pht_rp_stop_w(double w, double u, double num) { return (w < PHT_LLU_TINY) && (w * u < PHT_LLU_TINY * num); }

/* M(t) from the draw's cc column (invk[k] = 1 / k); *bad = 1 and NaN for a bad
 * evaluation; *khi = the upper end of the summation window */
PHT_HD double pht_rp_rmean(const double *cc, const double *invk, int K, double mu, double t, int *bad, int *khi) {
  const double lam = mu * t;
  const int lam_ok = (lam > 0.0) && (lam < INFINITY);
  const int k0 = (lam_ok && lam < (double)K) ? (int)floor(lam) : K;
  const double il = 1.0 / lam;
  const double ctop = cc[K];
  double num = cc[k0], den = 1.0, w = 1.0;
  for (int k = k0; k > 0;) {
    w = w * ((double)k * il);
    k--;
    if (pht_rp_stop_w(w, cc[k], num)) break;
    num = fma(w, cc[k], num);
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
    if (pht_rp_stop_w(w, ctop, num)) {
      k--;
      break;
    }
    num = fma(w, cc[k], num);
    den = den + w;
  }
  *khi = k;
  const double M = (num / den) / mu;
  const int ok = lam_ok && !tooshort && (M > 0.0) && (M < INFINITY);
  *bad = !ok;
  return ok ? M : NAN;
}

/* the three series at t; returns 1 if any is bad (the values are then NaN);
 * *khi = the largest upper window end */
PHT_HD int pht_rp_eval3(const double *tab, const double *cc, const double *invk, int K, double mu, double abar_x,
                        double t, double *lS, double *lf, double *M, int *khi) {
  int b1, b2, b3, k1, k2, k3;
  const double l1 = pht_llu_eval(tab, invk, K, mu, abar_x, t, 1, &b1, &k1);
  const double l2 = pht_llu_eval(tab, invk, K, mu, abar_x, t, 0, &b2, &k2);
  const double mm = pht_rp_rmean(cc, invk, K, mu, t, &b3, &k3);
  const int bad = b1 | b2 | b3;
  int k = (k1 > k2) ? k1 : k2;
  k = (k3 > k) ? k3 : k;
  *khi = k;
  *lS = bad ? NAN : l1;
  *lf = bad ? NAN : l2;
  *M = bad ? NAN : mm;
  return bad;
}

/* one (draw, age) of the curve; returns the age's flag word */
PHT_HD unsigned pht_rp_curve(const double *tab, const double *cc, const double *invk, int K, double mu, double abar_x,
                             double thi, double tau, double *lS, double *lf, double *M) {
  if (!(tau <= thi)) {
    *lS = *lf = *M = NAN;
    return PHT_RP_A_BEYOND;
  }
  int khi;
  return pht_rp_eval3(tab, cc, invk, K, mu, abar_x, tau, lS, lf, M, &khi) ? PHT_RP_A_EVAL : 0u;
}

/* g and D from the curve's values */
PHT_HD double pht_rp_g(double lS, double M, double cp, double cf) { return (cp + (cf - cp) * pht_fc_q(lS)) / M; }
/* g as the argmin takes it: a NaN counts as +inf, so it never beats a number */
PHT_HD double pht_rp_gsel(double lS, double M, double cp, double cf) {
  const double g = pht_rp_g(lS, M, cp, cf);
  return (g == g) ? g : INFINITY;
}
PHT_HD double pht_rp_c0(double cp, double cf) { return cp / (cf - cp); }
PHT_HD double pht_rp_D(double lS, double lf, double M, double c0) {
  return (pht_exp(lf - lS) * M - pht_fc_q(lS)) - c0;
}

/* D at t from the series (*bad: NaN) */
PHT_HD double pht_rp_D_at(const double *tab, const double *cc, const double *invk, int K, double mu, double abar_x,
                          double t, double c0, int *bad) {
  double lS, lf, M;
  int khi;
  *bad = pht_rp_eval3(tab, cc, invk, K, mu, abar_x, t, &lS, &lf, &M, &khi);
  return *bad ? NAN : pht_rp_D(lS, lf, M, c0);
}

/* point i = 0 .. 64 of a multisection step on [a, b] (point 0 is a) */
PHT_HD double pht_rp_point(double a, double b, int i) { return a + ((double)i * (b - a)) / (double)(PHT_RP_NPT + 1); }

/* point i (1 .. 64) lies strictly above its predecessor, the last one strictly below b */
PHT_HD int pht_rp_inside_i(double a, double b, int i) {
  const double t = pht_rp_point(a, b, i);
  return (t > pht_rp_point(a, b, i - 1)) && (i < PHT_RP_NPT || t < b);
}

PHT_HD int pht_rp_inside(double a, double b) {
  for (int i = 1; i <= PHT_RP_NPT; i++)
    if (!pht_rp_inside_i(a, b, i)) return 0;
  return 1;
}

PHT_HD int pht_rp_stop(double a, double b) { return (b - a <= PHT_RP_RTOL * b) || pht_q_adjacent(a, b); }

PHT_HD void pht_rp_set(pht_rp_out_t *o, double t, double g, double lo, double hi, int j, int nev, unsigned flags) {
  o->t = t;
  o->g = g;
  o->lo = lo;
  o->hi = hi;
  o->j = j;
  o->nev = nev;
  o->flags = flags;
}

/* step 5 on a finite candidate */
PHT_HD void pht_rp_finish(pht_rp_out_t *o, double t, double g, double lo, double hi, int j, int nev, unsigned flags,
                          double ginf) {
  if (ginf <= g)
    pht_rp_set(o, INFINITY, ginf, lo, hi, j, nev, flags | PHT_RP_F_NEVER);
  else
    pht_rp_set(o, t, g, lo, hi, j, nev, flags);
}

/* Step 2 from the argmin j and the last good age jlast: returns 1 with the
 * bracket [*a, *b] to refine, or 0 with *flags = PHT_RP_F_EDGE or
 * PHT_RP_F_UNREFINED (the result is tau_j). */
PHT_HD int pht_rp_bracket(int G, const double *ages, const double *lS, const double *lf, const double *M,
                          const unsigned *aflags, int j, int jlast, double c0, double *a, double *b,
                          unsigned *flags) {
  const double Dj = pht_rp_D(lS[j], lf[j], M[j], c0);
  *flags = 0u;
  *a = *b = ages[j];
  if (Dj >= 0.0) {
    if (j == 0) {
      *a = 0.0;
      return 1;
    }
    if (aflags[j - 1] == 0u && pht_rp_D(lS[j - 1], lf[j - 1], M[j - 1], c0) < 0.0) {
      *a = ages[j - 1];
      return 1;
    }
    *flags = PHT_RP_F_UNREFINED;
    return 0;
  }
  if (j >= jlast) {
    *flags = PHT_RP_F_EDGE;
    return 0;
  }
  if (j + 1 < G && aflags[j + 1] == 0u && pht_rp_D(lS[j + 1], lf[j + 1], M[j + 1], c0) >= 0.0) {
    *b = ages[j + 1];
    return 1;
  }
  *flags = PHT_RP_F_UNREFINED;
  return 0;
}

/* one (draw, cost pair) of a usable draw from its curve: steps 1 to 5 */
PHT_HD void pht_rp_policy(const double *tab, const double *cc, const double *invk, int K, double mu, double abar_x,
                          double m, int G, const double *ages, const double *lS, const double *lf, const double *M,
                          const unsigned *aflags, double cp, double cf, pht_rp_out_t *o) {
  if (!pht_rp_cost_ok(cp, cf)) {
    pht_rp_set(o, NAN, NAN, NAN, NAN, -1, 0, PHT_RP_F_COST);
    return;
  }
  /* 1. the grid's argmin */
  int j = -1, jlast = -1;
  double gj = INFINITY;
  for (int i = 0; i < G; i++) {
    if (aflags[i]) continue;
    const double g = pht_rp_gsel(lS[i], M[i], cp, cf);
    jlast = i;
    if (j < 0 || g < gj) {
      j = i;
      gj = g;
    }
  }
  if (j < 0) {
    pht_rp_set(o, NAN, NAN, NAN, NAN, -1, 0, PHT_RP_F_NOAGE);
    return;
  }
  const double ginf = cf / m, c0 = pht_rp_c0(cp, cf);
  /* 2. the bracket */
  double a, b;
  unsigned fl;
  if (!pht_rp_bracket(G, ages, lS, lf, M, aflags, j, jlast, c0, &a, &b, &fl)) {
    pht_rp_finish(o, ages[j], gj, ages[j], ages[j], j, 0, fl, ginf);
    return;
  }
  /* 3. the refinement */
  int nev = 0, step = 0, bad;
  while (!pht_rp_stop(a, b)) {
    if (step >= PHT_RP_MAXSTEP) {
      pht_rp_set(o, NAN, NAN, a, b, j, nev, PHT_RP_F_CAP);
      return;
    }
    step++;
    if (pht_rp_inside(a, b)) {
      int first = 0, anybad = 0;
      for (int i = 1; i <= PHT_RP_NPT; i++) {
        const double d = pht_rp_D_at(tab, cc, invk, K, mu, abar_x, pht_rp_point(a, b, i), c0, &bad);
        anybad |= bad;
        if (!first && !bad && d >= 0.0) first = i;
      }
      nev += PHT_RP_NPT;
      if (anybad) {
        pht_rp_set(o, NAN, NAN, a, b, j, nev, PHT_RP_F_EVAL);
        return;
      }
      const double na = pht_rp_point(a, b, first ? first - 1 : PHT_RP_NPT);
      const double nb = first ? pht_rp_point(a, b, first) : b;
      a = na;
      b = nb;
    } else {
      const double t = pht_q_mid(a, b);
      const double d = pht_rp_D_at(tab, cc, invk, K, mu, abar_x, t, c0, &bad);
      nev++;
      if (bad) {
        pht_rp_set(o, NAN, NAN, a, b, j, nev, PHT_RP_F_EVAL);
        return;
      }
      if (d >= 0.0)
        b = t;
      else
        a = t;
    }
  }
  /* 4. the result */
  double th = a + 0.5 * (b - a);
  th = (th < a) ? a : ((th > b) ? b : th);
  double l1, l2, mm;
  int khi;
  bad = pht_rp_eval3(tab, cc, invk, K, mu, abar_x, th, &l1, &l2, &mm, &khi);
  nev++;
  if (bad) {
    pht_rp_set(o, NAN, NAN, a, b, j, nev, PHT_RP_F_EVAL);
    return;
  }
  pht_rp_finish(o, th, pht_rp_g(l1, mm, cp, cf), a, b, j, nev, 0u, ginf);
}

/* what a flagged draw gives for every pair */
PHT_HD void pht_rp_flagged(pht_rp_out_t *o) { pht_rp_set(o, NAN, NAN, NAN, NAN, -1, 0, PHT_RP_F_DRAW); }

/* The whole function for one draw on the host (no device): the curve on G
 * ages (pht_rp_ages_ok) and P policies of (S column-major n x n, s), n <= 32.
 * work: PHT_RP_WORK(G) doubles (tab, cc, invk, then lS, lf, M of G each: the
 * curve is left there); aflags: G words, written; lS_out, lf_out, M_out (each
 * G) may be null; t, g, lo, hi, j, nev, flags: P each, written; *m_out: E[T]
 * (NaN for a flagged draw).  Returns the draw's flag word. */
PHT_HD unsigned pht_rp_draw(int n, const double *S, const double *s, int G, const double *ages, int P,
                            const double *cp, const double *cf, double *work, unsigned *aflags, double *lS_out,
                            double *lf_out, double *M_out, double *m_out, double *t, double *g, double *lo,
                            double *hi, int *j, int *nev, unsigned *flags) {
  const int rows = PHT_LLU_MAXK + 1;
  double *tab = work, *cc = work + 2 * rows, *invk = work + 3 * rows;
  double *lS = work + 4 * rows, *lf = lS + G, *M = lf + G;
  double meta[PHT_LLU_META], thi, m;
  const unsigned flag = pht_rp_meta(n, S, s, ages[G - 1], meta, &thi, &m);
  const int K = (int)meta[PHT_LLU_M_K];
  const double mu = meta[PHT_LLU_M_MU], abar = meta[PHT_LLU_M_ABAR];
  *m_out = m;
  if (!flag) {
    pht_llu_table(n, S, s, mu, K, tab);
    pht_rp_cc(tab, K, cc);
    for (int k = 0; k <= K; k++) invk[k] = k ? 1.0 / (double)k : 0.0;
  }
  for (int i = 0; i < G; i++) {
    if (flag) {
      lS[i] = lf[i] = M[i] = NAN;
      aflags[i] = PHT_RP_A_DRAW;
    } else {
      aflags[i] = pht_rp_curve(tab, cc, invk, K, mu, abar, thi, ages[i], &lS[i], &lf[i], &M[i]);
    }
    if (lS_out) lS_out[i] = lS[i];
    if (lf_out) lf_out[i] = lf[i];
    if (M_out) M_out[i] = M[i];
  }
  for (int p = 0; p < P; p++) {
    pht_rp_out_t o;
    if (flag)
      pht_rp_flagged(&o);
    else
      pht_rp_policy(tab, cc, invk, K, mu, abar, m, G, ages, lS, lf, M, aflags, cp[p], cf[p], &o);
    t[p] = o.t;
    g[p] = o.g;
    lo[p] = o.lo;
    hi[p] = o.hi;
    j[p] = o.j;
    nev[p] = o.nev;
    flags[p] = o.flags;
  }
  return flag;
}

#endif /* PHT_REPLACE_H */
