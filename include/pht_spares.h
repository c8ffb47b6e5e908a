/*
 * pht_spares.h — specification of the fleet spares: for every posterior draw
 * (S, s) with pi = e_1, every unit still in service at age c_i (a
 * right-censored observation) and every horizon h, the MEAN and the VARIANCE of
 * the number N(h) of failures within h when a failed unit is replaced by a new
 * one.  include/pht_condition.h gives the mean alone (D); nobody stocks spares
 * to the mean.  No reference counterpart.  Shared by the HIP kernels
 * (phasetype_amd/csrc/pht_spares.hip), the host (host_spares.cpp) and the
 * tests' CPU restatement (tests/spares_spec.c).  pht_condition.h is included
 * and not changed.
 *
 * The failures of a unit replaced at failure form a Markovian arrival process
 * with D0 = S, D1 = s e_1^T, Q* = S + s e_1^T.  From phase i,
 *   M1(h) = E_i N(h)            is r_h, pht_cd_renewal's column,
 *   M2(h) = E_i N(h) (N(h) - 1) satisfies M2' = Q* M2 + 2 s M1[0]
 * (a failure at u lands in phase 1 and pairs with every later one).
 * Uniformised with pht_cd_renewal's mu and P*, with c = s rinv:
 *   b_0 = a_0 = 0,  b_{k+1} = P* b_k + c,  a_{k+1} = P* a_k + 2 c b_k[0],
 *   q_h = sum_{k=0..Kr} p_k a_k,   p_k the Poisson(mu h) weight
 * (b_k = E_i[jumps of the uniformised chain that are failures, among its first
 * k], a_k its second factorial moment).  Every term is non-negative.
 *
 * Per draw (pht_sp_vectors).  Kr = pht_llu_K(mu, h_max).  Per horizon j the
 * weights of pht_cd_renewal, operation for operation (lam = mu h_j, k0, il,
 * w_k0 = 1, down, up, den), and from the suffix sum from the top, acc = 0, for
 * k = Kr .. 0:
 *     T_k = acc / den,  p_k = w_k / den,  acc = acc + w_k.
 * They are kept as W[(k nh + j) 2 + {0, 1}] = (T_k, p_k) (PHT_SP_W), w_k in the
 * T slot until the suffix sum replaces it.  Then with P* as pht_cd_renewal
 * builds it, c_i = s_i rinv (the product P*[i][0] already holds) and
 * c2_i = 2 c_i (exact), u_0 = s, a_0 = b_0 = 0, for k = 0 .. Kr:
 *   if k > 0, from the vectors of k - 1 and for every row i (j increasing)
 *     u_k[i] = sum_j fma(P*[i][j], u[j], .)                   from 0
 *     a_k[i] = sum_j fma(P*[i][j], a[j], .)                   from c2_i b[0]
 *     b_k[i] = sum_j fma(P*[i][j], b[j], .)                   from c_i
 *   then for every horizon j
 *     r_j[i] = fma(T_k, u_k[i], r_j[i]),  q_j[i] = fma(p_k, a_k[i], q_j[i])
 * and at the end r_j[i] = rinv r_j[i] (q_j is a count: no factor).  r_j is BIT
 * FOR BIT pht_cd_renewal's: the same P*, T_k, fma order per row, k increasing.
 * h_j = 0 gives T = 0, p_0 = 1 and r_j = q_j = 0 exactly.
 *
 *   Scales: dscale_j = pht_es_yscale(max_i r_j[i]) (the condition's) and
 *   vscale_j = pht_es_yscale(max_i (q_j[i] + r_j[i])): powers of two that
 *   depend on the draw only, so that shards' words add.
 *
 * Per (draw, unit) at age c: the window and phi exactly as in pht_cd_draw
 * (pht_es_window, pht_cd_phase, pht_cd_phi).  Then per horizon
 *   D = pht_cd_dot(phi, r_j),  Q = pht_cd_dot(phi, q_j),
 *   var = fmax(fma(-D, D, Q + D), 0)                          (pht_sp_var)
 * Var N = E N (N - 1) + E N - (E N)^2.  Q + D rounds once, the fma once; the
 * truth is non-negative, so a negative value is rounding alone and is cut.  At
 * h = 0: D = Q = 0 and var = 0 exactly.  var <= Q + D = phi . (q_j + r_j) <=
 * vscale_j up to n + 2 roundings.  A bad unit is counted, never summed, NaN
 * pointwise.
 *
 * Flags are the condition's, so that the same draws are skipped as by
 * pht_cd_draw for the same input: pht_llu_meta's, PHT_CD_F_TRAP from
 * pht_cd_mean (m itself is not used) and PHT_CD_F_HCAP where Kr reaches
 * PHT_LLU_MAXK (pht_sp_flags: nothing with a Kr factor).
 *
 * Measured constants (against mpmath, exp of the augmented generator
 * [[Q*, 2 s e_1^T, 0], [0, Q*, s], [0, 0, 0]] at 60 digits and more), on
 * bd_exit(3), bd_exit(10), Erlang(3), ring(5) and stiff(6), horizons
 * 1e-6 .. 1e3 / mu, margin four: these five sample the growth, they do not
 * bound it (pht_condition.h's method for PHT_CD_R_R).
 *   |q^_h[i] - q_h[i]| <= PHT_SP_Q_R (mu h + 8) q_h[i]          (pht_sp_q_bound)
 *     PHT_SP_Q_R = 3.2 x 2^-53; largest measured ratio on the five 0.80
 *     (bd_exit(10), mu h = 1e-3); at mu h = 1000 measured 4.4 .. 190 x 2^-53,
 *     stiff(6) the largest
 *   a unit's variance loses what Q + D - D^2 cancels: with E = Q + D + D^2,
 *   |var^ - var| <= PHT_SP_V_R (mu h + 8) E + the error phi itself carries
 *     PHT_SP_V_R = 3.6 x 2^-53 (pht_sp_var_bound; the tests measure var with
 *     phi = e_i exact, i.e. on the columns: largest measured ratio on the five
 *     0.89, stiff(6), mu h = 1; at mu h = 1000 the error is 68 .. 281 x 2^-53 E,
 *     Erlang(3) the largest, where D = 334 and var loses 5.6e5 x 2^-53 of itself)
 *   so the relative error of var is about ulp (mu h) D^2 / var: a few digits
 *   are lost at D in the hundreds.
 * Measured since on ten more generators, the bidiagonal chains among them
 * (acyclic, reversible, nearly equal, Erlang, shared-rate Coxian, gapped and
 * hypoexponential at n = 6, hypoexp(10), acyclic(12), stiff(12); the truth at
 * 60 + 6 n max(0, -log10(mu h)) + mu h / 2.3 digits, since q_h[i] is as small
 * as (mu h)^(2 n - i) there): the constants hold, with less than the margin of
 * four.  Largest measured ratio over all fifteen: q_h 2.81 (0.88 of the
 * bound) and var 1.76 (0.49 of the bound), both hypoexp(10) at mu h = 0.1;
 * hypoexp(6) 1.61 and gapped(6) 1.35 for q_h at mu h = 0.01; every other
 * generator stays below 1.0 in both.
 * (tests/test_spares.py gates both on the same grid, on all fifteen.)
 *
 * Exact reductions.  Per draw pht_sp_nwords(nh) = 2 nh + 2 int64 words over the
 * units good for that draw,
 *   [Delta_0 .. Delta_{nh-1}, V_0 .. V_{nh-1}, nbad, nunits],
 *   Delta_h = sum_i llrint((D / dscale_h) 2^40)   (the condition's word),
 *   V_h     = sum_i llrint((var / vscale_h) 2^40).
 * At most PHT_CD_MAXUNITS = 2^22 units, so every sum is at most 2^62.  Units
 * are independent given the draw: V_h is the fleet's within-draw variance.
 *
 * Per unit, IN DRAW ORDER (x <- x + value): dsum[nh], vsum[nh], d2sum[nh] (the
 * sum of D D, one rounded product each) and cnt.
 *
 * Limits: n <= 32; 1 <= nh <= PHT_CD_MAXH = 16 horizons that pass
 * pht_fc_horizons_ok (nh = 0 is refused: there is nothing to compute).
 *
 * Every operation is explicit; every unit that includes this is compiled with
 * -ffp-contract=off; divisions are IEEE.  A GPU lane and the CPU restatement
 * give the same bits.
 */
#ifndef PHT_SPARES_H
#define PHT_SPARES_H

#include "pht_condition.h"

#define PHT_SP_Q_R (3.2 * 0x1p-53) /* measured relative error bound of q_h, times (mu h + 8), margin 4 */
#define PHT_SP_V_R (3.6 * 0x1p-53) /* that of var relative to Q + D + D^2, times (mu h + 8), margin 4 */

/* doubles of the weights of one draw with rows = Kr + 1, and where (T_k, p_k) of horizon j are */
#define PHT_SP_WDOUBLES(nh, rows) ((size_t)2 * (size_t)(nh) * (size_t)(rows))
#define PHT_SP_W(nh, k, j) (((size_t)(k) * (size_t)(nh) + (size_t)(j)) * 2)

/* doubles of pht_sp_draw's workspace: tab, invk, F and the weights W */
#define PHT_SP_WORK(n, nh) ((size_t)(3 + (n) + 2 * (nh)) * (PHT_LLU_MAXK + 1))

/* words per draw, and where they are */
PHT_HD int pht_sp_nwords(int nh) { return 2 * nh + 2; }
PHT_HD int pht_sp_w_D(int j) { return j; }
PHT_HD int pht_sp_w_V(int nh, int j) { return nh + j; }
PHT_HD int pht_sp_w_nbad(int nh) { return 2 * nh; }
PHT_HD int pht_sp_w_nunits(int nh) { return 2 * nh + 1; }

/* 1 .. 16 horizons by the forecast's rule */
PHT_HD int pht_sp_horizons_ok(int nh, const double *h) {
  return (nh >= 1) && (nh <= PHT_CD_MAXH) && pht_fc_horizons_ok(nh, h);
}

/* the recorded relative bound of q_h at lam = mu h */
PHT_HD double pht_sp_q_bound(double lam) { return PHT_SP_Q_R * (lam + 8.0); }
/* the recorded absolute bound of var given exact phi, from the truths D and Q */
PHT_HD double pht_sp_var_bound(double lam, double D, double Q) { return (PHT_SP_V_R * (lam + 8.0)) * (Q + D + D * D); }

/* the specification's own two flags of a draw that pht_llu_meta passed (0:
 * usable): the condition's, at no cost in Kr */
PHT_HD unsigned pht_sp_flags(int n, const double *S, const double *s, double mu, double hmax) {
  double m[32];
  unsigned flag = pht_cd_mean(n, S, s, m);
  if (pht_llu_K(mu, hmax) >= PHT_LLU_MAXK) flag |= PHT_CD_F_HCAP;
  return flag;
}

/* (T_k, p_k), k = 0 .. Kr, of horizon j of nh into W (PHT_SP_W): the weights
 * of pht_cd_renewal, operation for operation.  One GPU lane runs this per
 * horizon. */
PHT_HD void pht_sp_weights(double mu, double hj, int Kr, int nh, int j, double *W) {
  const double lam = mu * hj;
  const int k0 = (lam < (double)Kr) ? (int)floor(lam) : Kr;
  const double il = 1.0 / lam;
  double den = 1.0, x = 1.0;
  W[PHT_SP_W(nh, k0, j)] = 1.0;
  for (int k = k0; k > 0;) {
    x = x * ((double)k * il);
    k--;
    W[PHT_SP_W(nh, k, j)] = x;
    den = den + x;
  }
  x = 1.0;
  for (int k = k0; k < Kr;) {
    k++;
    x = x * (lam * (1.0 / (double)k));
    W[PHT_SP_W(nh, k, j)] = x;
    den = den + x;
  }
  double acc = 0.0;
  for (int k = Kr; k >= 0; k--) {
    double *w = W + PHT_SP_W(nh, k, j);
    const double wk = w[0];
    w[0] = acc / den;
    w[1] = wk / den;
    acc = acc + wk;
  }
}

/* the variance of a unit's count from its D and Q */
PHT_HD double pht_sp_var(double D, double Q) { return fmax(fma(-D, D, Q + D), 0.0); }

/* one usable draw's vectors: r[j n + i] = r_{h_j}[i], q[j n + i] = q_{h_j}[i],
 * scales[2 nh] = [dscale_j, vscale_j] (nh >= 1, the horizons ok,
 * pht_llu_K(mu, h_max) < PHT_LLU_MAXK).  W: PHT_SP_WDOUBLES(nh, Kr + 1). */
PHT_HD void pht_sp_vectors(int n, const double *S, const double *s, double mu, int nh, const double *h, double *W,
                           double *r, double *q, double *scales) {
  const int Kr = pht_llu_K(mu, h[nh - 1]);
  const double rinv = 1.0 / mu;
  for (int j = 0; j < nh; j++) pht_sp_weights(mu, h[j], Kr, nh, j, W);
  double P[32 * 32], c[32], c2[32], u[32], a[32], b[32], un[32], an[32], bn[32];
  for (int i = 0; i < n; i++) {
    for (int j = 0; j < n; j++) P[i * n + j] = pht_llu_R(S[i + j * n], rinv, i == j);
    c[i] = s[i] * rinv;
    c2[i] = 2.0 * c[i];
    P[i * n] = P[i * n] + c[i];
    u[i] = s[i];
    a[i] = 0.0;
    b[i] = 0.0;
  }
  for (int j = 0; j < nh * n; j++) r[j] = q[j] = 0.0;
  for (int k = 0; k <= Kr; k++) {
    if (k) {
      const double b0 = b[0];
      for (int i = 0; i < n; i++) {
        double vu = 0.0, va = c2[i] * b0, vb = c[i];
        for (int j = 0; j < n; j++) {
          vu = fma(P[i * n + j], u[j], vu);
          va = fma(P[i * n + j], a[j], va);
          vb = fma(P[i * n + j], b[j], vb);
        }
        un[i] = vu;
        an[i] = va;
        bn[i] = vb;
      }
      for (int i = 0; i < n; i++) {
        u[i] = un[i];
        a[i] = an[i];
        b[i] = bn[i];
      }
    }
    for (int j = 0; j < nh; j++) {
      const double *w = W + PHT_SP_W(nh, k, j);
      for (int i = 0; i < n; i++) {
        r[j * n + i] = fma(w[0], u[i], r[j * n + i]);
        q[j * n + i] = fma(w[1], a[i], q[j * n + i]);
      }
    }
  }
  for (int j = 0; j < nh * n; j++) r[j] = rinv * r[j];
  for (int j = 0; j < nh; j++) {
    double mr = 0.0, mv = 0.0;
    for (int i = 0; i < n; i++) {
      const double x = r[j * n + i], y = q[j * n + i] + x;
      mr = (x > mr) ? x : mr;
      mv = (y > mv) ? y : mv;
    }
    scales[j] = pht_es_yscale(mr);
    scales[nh + j] = pht_es_yscale(mv);
  }
}

/* The whole specification for one draw on the host (no device): ncens units
 * of ages c, nh horizons (pht_sp_horizons_ok), the tables sized for ymax_c.
 * work: PHT_SP_WORK(n, nh) doubles.  words [pht_sp_nwords], scales [2 nh]:
 * written (zero for a flagged draw).  dsum, vsum, d2sum [ncens][nh], cnt
 * [ncens]: UPDATED (the draws of a chain in order: one call each); dd, var
 * [ncens][nh]: written (NaN where bad); each of the six may be null.  Returns
 * the draw's flag word. */
PHT_HD unsigned pht_sp_draw(int n, const double *S, const double *s, long ncens, const double *c, double ymax_c, int nh,
                            const double *h, double *work, long long *words, double *scales, double *dsum, double *vsum,
                            double *d2sum, long long *cnt, double *dd, double *var) {
  double meta[PHT_LLU_META], r[PHT_CD_MAXH * 32], q[PHT_CD_MAXH * 32], v[32];
  double *tab = work, *invk = tab + 2 * (PHT_LLU_MAXK + 1), *F = invk + (PHT_LLU_MAXK + 1);
  double *W = F + (size_t)n * (PHT_LLU_MAXK + 1);
  const int nw = pht_sp_nwords(nh);
  unsigned flag = pht_llu_meta(n, S, s, ymax_c, meta);
  for (int j = 0; j < nw; j++) words[j] = 0;
  for (int j = 0; j < 2 * nh; j++) scales[j] = 0.0;
  const double mu = meta[PHT_LLU_M_MU], abar = meta[PHT_LLU_M_ABAR];
  if (!flag) flag = pht_sp_flags(n, S, s, mu, h[nh - 1]);
  if (flag) {
    for (long i = 0; i < ncens; i++)
      for (int j = 0; j < nh; j++) {
        if (dd) dd[i * nh + j] = NAN;
        if (var) var[i * nh + j] = NAN;
      }
    return flag;
  }
  pht_sp_vectors(n, S, s, mu, nh, h, W, r, q, scales);
  const int K = (int)meta[PHT_LLU_M_K];
  pht_llu_table(n, S, s, mu, K, tab);
  pht_cd_forward(n, S, mu, K, F);
  for (int k = 0; k <= K; k++) invk[k] = k ? 1.0 / (double)k : 0.0;
  for (long i = 0; i < ncens; i++) {
    int bad;
    pht_es_win_t win;
    (void)pht_es_window(tab, invk, K, mu, abar, c[i], 1, &bad, &win);
    if (bad) {
      words[pht_sp_w_nbad(nh)] += 1;
      for (int j = 0; j < nh; j++) {
        if (dd) dd[i * nh + j] = NAN;
        if (var) var[i * nh + j] = NAN;
      }
      continue;
    }
    pht_cd_phase(F, n, n, invk, &win, v);
    pht_cd_phi(n, n, v);
    for (int j = 0; j < nh; j++) {
      const double dv = pht_cd_dot(n, n, v, r + j * n);
      const double qv = pht_cd_dot(n, n, v, q + j * n);
      const double vv = pht_sp_var(dv, qv);
      words[pht_sp_w_D(j)] += pht_cd_fixed_scaled(dv, scales[j]);
      words[pht_sp_w_V(nh, j)] += pht_cd_fixed_scaled(vv, scales[nh + j]);
      if (dsum) dsum[i * nh + j] = dsum[i * nh + j] + dv;
      if (vsum) vsum[i * nh + j] = vsum[i * nh + j] + vv;
      if (d2sum) d2sum[i * nh + j] = d2sum[i * nh + j] + dv * dv;
      if (dd) dd[i * nh + j] = dv;
      if (var) var[i * nh + j] = vv;
    }
    words[pht_sp_w_nunits(nh)] += 1;
    if (cnt) cnt[i] += 1;
  }
  return flag;
}

#endif /* PHT_SPARES_H */
