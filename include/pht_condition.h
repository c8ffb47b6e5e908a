/*
 * pht_condition.h — specification of the fleet condition: for every posterior
 * draw (S, s) with pi = e_1 and every unit still in service at age c_i (a
 * right-censored observation), the posterior law of the PHASE the unit is in,
 *   phi_i = e_1^T exp(S c_i) / (e_1^T exp(S c_i) 1),
 * and the two functionals of it that a fleet's owner asks for: the mean
 * residual life MRL_i = phi_i . m, m = (-S)^-1 1, and the expected number of
 * failures within h when a failed unit is replaced by a new one,
 * D_i(h) = phi_i . r_h, r_h = int_0^h exp(Q* u) s du, Q* = S + s e_1^T (the
 * failures form a Markovian arrival process; the count does not saturate at
 * one a unit as include/pht_forecast.h's first-failure probability does).
 * With their exact sums over the units per draw and over the draws per unit.
 * No reference counterpart.  Shared by the HIP kernels
 * (phasetype_amd/csrc/pht_condition.hip), the host (host_condition.cpp) and
 * the tests' CPU restatement (tests/condition_spec.c).
 *
 * Per draw.  The meta words of pht_llu_meta and the table of pht_llu_table
 * (include/pht_loglik_unif.h, unchanged), sized for ymax_c, the largest
 * CENSORED observation of the context (ages only: no horizon is added, the
 * horizons never enter a unit's window).  The evaluator's limits are
 * inherited: pi = e_1 and K <= 2047.  A draw with a flag (pht_llu_meta's, or
 * one of the two below) is skipped: its words and scales are zero, its
 * pointwise values NaN, and no unit's sums or cnt move.
 *
 *   Forward table (pht_cd_forward).  F[k][j], k = 0..K: f_0 = e_1,
 *     f_k[j] = sum_l fma(f_{k-1}[l], R[l][j], .)      (l increasing, from 0)
 *   with R of pht_llu_R: pht_es_contract's advance, operation for operation.
 *   sum_j f_k[j] = ac_k up to rounding, and f_k[j] <= ac_k.
 *
 *   Mean-time vector (pht_cd_mean), (-S) m = 1, by elimination without
 *   pivoting in a subtraction-free (GTH) form.  Working on copies of the
 *   off-diagonal rates A_ij = S_ij, the exit rates e_i = s_i and b_i = 1, for
 *   k = n - 1 down to 1:
 *     d_k = e_k, then d_k = d_k + A_kj for j = 0 .. k - 1 (j increasing)
 *     for i = 0 .. k - 1:  t = A_ik / d_k,
 *       A_ij = fma(t, A_kj, A_ij)  for j = 0 .. k - 1, j != i,
 *       e_i = fma(t, e_k, e_i),  b_i = fma(t, b_k, b_i)
 *   and d_0 = e_0; then m_0 = b_0 / d_0 and for k = 1 .. n - 1
 *     m_k = (b_k + sum_{j<k} fma(A_kj, m_j, .)) / d_k   (j increasing; the sum
 *   starts from b_k).  The diagonal of S is never read: each pivot is rebuilt
 *   as the sum of the row's remaining rates and its exit rate, every number is
 *   non-negative and nothing cancels.  A pivot that is not positive and finite
 *   means a state that cannot reach absorption: PHT_CD_F_TRAP.
 *
 *   Renewal columns (pht_cd_renewal), only when nh > 0.  P* = R with
 *   P*[i][0] = R[i][0] + s_i rinv (the uniformised Q*, a stochastic matrix),
 *   u_0 = s, u_k[i] = sum_j fma(P*[i][j], u_{k-1}[j], .) (j increasing), and
 *     r_h = (1 / mu) sum_k P(N > k) u_k,   N ~ Poisson(mu h).
 *   Kr = pht_llu_K(mu, h_max), h_max the last horizon; if the sizing rule
 *   reaches the cap (Kr = PHT_LLU_MAXK, mu h_max from about 1450) the draw
 *   gets PHT_CD_F_HCAP and is skipped as a whole, so that there is one cnt a
 *   unit.  For horizon j: lam = mu h_j, k0 = min(floor(lam), Kr), il = 1 / lam,
 *   the Poisson weights relative to the mode as pht_llu_eval builds them
 *   (w_k0 = 1; down w_{k-1} = w_k (k il), den = den + w; up
 *   w_k = w_{k-1} (lam (1 / k))), over ALL of 0 .. Kr (no stop rule: a weight
 *   that underflows is zero); the tails by a suffix sum from the top,
 *   acc = 0, for k = Kr .. 0: T_k = acc / den, acc = acc + w_k; and
 *     r_j[i] = rinv * sum_{k=0..Kr} fma(T_k, u_k[i], .)     (k increasing).
 *   Every term is non-negative.  h_j = 0 gives r_j = 0 exactly.
 *
 *   Scales: mscale = pht_es_yscale(max_j m_j), dscale_j =
 *   pht_es_yscale(max_i r_j[i]): powers of two that depend on the draw only,
 *   so that shards' words add.
 *
 * Per (draw, unit) at age c:
 *   l = pht_es_window(tab, invk, K, mu, abar, c, cens = 1, &bad, &win):
 *   bit for bit loglik_unif's pointwise value and the forecast's l0, and bad
 *   is the forecast's at that age.  A second pass (pht_cd_phase) runs the same
 *   w_k recurrence from k0 as pht_es_obs does: v[j] = F[k0][j]; downward to
 *   klo and then upward to khi, v[j] = fma(w_k, F[k][j], v[j]).  Then
 *   (pht_cd_phi) tot = sum_j v[j] (j increasing, from v[0]),
 *   phi_j = v_j / tot (IEEE divisions by the vector's own sum, so sum phi = 1
 *   to rounding), MRL = sum_j fma(phi_j, m_j, .) and
 *   D_h = sum_j fma(phi_j, r_h[j], .) (pht_cd_dot: from 0, j increasing).
 *   A bad unit is counted, never summed, and NaN pointwise.
 *
 * Contract for phi.  Everything is a sum of non-negative terms.  One term
 * w_k f_k[j]: f_k[j] comes from k matrix-vector steps of length n
 * ((n + 2) k roundings), w_k from at most 3 |k - k0| roundings (lam and il
 * once, two products a step), and v_j is one more sum of W = khi - klo + 1
 * terms: at most (n + 5) (khi + 1) + W <= (n + 9) (khi + 1) roundings, relative
 * to v_j itself.  tot carries the same and n - 1 additions, the quotient one
 * more.  Truncation: f_k[j] <= ac_k, so what the window leaves out of v_j is
 * at most what the censored column's stop rule leaves out of num: 2^-57 num
 * (pht_loglik_unif.h's 2^-56 is for the two sums), and num = tot up to the
 * rounding above; v_j and tot each lose at most that, which moves the
 * quotient by at most (2^-57 + phi_j 2^-57) <= 2^-56.  So
 *   |phi^_j - phi_j| <= 2^-53 (2 (n + 9) (khi + 1) + n + 2) phi_j + 2^-56
 * (pht_cd_phi_bound; phi_j the truth).  cond(Q) does not enter.
 *
 * m and r_h.  The elimination's relative error grows with the expected number
 * of visits to a state, which depends on the generator; the recorded
 * constants are MEASURED against mpmath (60 digits) on bd_exit(3),
 * bd_exit(10), Erlang(3), ring(5) and stiff(6), horizons 1e-6 .. 1e3 / mu, and
 * carry a margin of four: these five sample the growth and do not bound it.
 *   |m^_j - m_j| <= PHT_CD_M_R m_j,  PHT_CD_M_R = 21 x 2^-53
 *     largest measured: 5.11 x 2^-53 (ring(5); bd_exit(10) 3.30, bd_exit(3) 2.63)
 *   |r^_h[i] - r_h[i]| <= PHT_CD_R_R (mu h + 8) r_h[i],  PHT_CD_R_R = 3.5 x 2^-53
 *     (pht_cd_r_bound) the error grows with the rows that carry weight, mu h:
 *     at mu h = 1000 measured 83 .. 282 x 2^-53, at mu h = 100 6.3 .. 26.5, below
 *     mu h = 1 at most 7.5; largest measured ratio on the five 0.83 (stiff(6),
 *     mu h = 1)
 * Measured since on ten more generators, the bidiagonal chains among them
 * (acyclic, reversible, nearly equal, Erlang, shared-rate Coxian, gapped and
 * hypoexponential at n = 6, hypoexp(10), acyclic(12), stiff(12); r_h's truth
 * at 60 + 3 n max(0, -log10(mu h)) + mu h / 2.3 digits, since r_h[i] is as
 * small as (mu h)^(n - i) there): the constants hold, r_h with less than the
 * margin of four.  m: at most 3.49 x 2^-53 (acyclic(12)), ring(5)'s 5.11 stays
 * the largest.  r_h: largest measured ratio over all fifteen 1.68 (0.48 of the
 * bound), hypoexp(10) at mu h = 0.1, 13.6 x 2^-53 where the five gave at most
 * 7.5; hypoexp(6) 0.92 at mu h = 0.01.  phi stays within 0.026 of its contract.
 * (tests/test_condition.py gates both on the same grid, on all fifteen.)
 *
 * Exact reductions.  Per draw pht_cd_nwords(n, nh) = n + nh + 3 int64 words
 * over the units good for that draw,
 *   [Phi_0 .. Phi_{n-1}, L, Delta_0 .. Delta_{nh-1}, nbad, nunits],
 *   Phi_j = sum_i llrint(phi_j 2^40)   the expected number of units in phase j,
 *   L = sum_i llrint((MRL / mscale) 2^40),
 *   Delta_h = sum_i llrint((D_h / dscale_h) 2^40).
 * At most PHT_CD_MAXUNITS = 2^22 censored units per context, so every sum is
 * at most 2^62 (MRL <= mscale and D_h <= dscale_h up to n roundings).  Integer
 * sums: they depend on neither the grid, the batch nor the shard.
 *
 * Per unit, IN DRAW ORDER (x <- x + value): phisum[n], mrlsum, dsum[nh], and
 * cnt, the number of draws in which the unit was good.
 *
 * Limits: n <= 32; 0 <= nh <= PHT_CD_MAXH = 16 horizons, which pass
 * pht_fc_horizons_ok when nh > 0.
 *
 * Every operation is explicit; every unit that includes this is compiled with
 * -ffp-contract=off; exp and log are include/pht_detmath.h's; divisions and
 * sqrt are IEEE.  A GPU lane and the CPU restatement give the same bits.
 */
#ifndef PHT_CONDITION_H
#define PHT_CONDITION_H

#include "pht_estep.h"
#include "pht_forecast.h"
#include "pht_loglik_unif.h"

#define PHT_CD_F_TRAP 64u  /* a state that cannot reach absorption (a pivot not positive and finite) */
#define PHT_CD_F_HCAP 128u /* mu h_max beyond the renewal table's sizing rule */

#define PHT_CD_MAXH 16             /* horizons of a call (0 allowed) */
#define PHT_CD_MAXUNITS (1L << 22) /* censored units of a context */
#define PHT_CD_SCALE 0x1p40        /* the fixed point of the words */
#define PHT_CD_M_R (21.0 * 0x1p-53) /* measured relative error bound of m, margin 4 */
#define PHT_CD_R_R (3.5 * 0x1p-53)  /* that of r_h, times (mu h + 8), margin 4 */

/* the per-unit loops over the phases are unrolled where the caller's nmax is
 * a compile-time constant (the kernel: v stays in registers) */
#if defined(__clang__)
#define PHT_CD_UNROLL _Pragma("unroll")
#else
#define PHT_CD_UNROLL
#endif

/* doubles of pht_cd_draw's workspace: tab, invk, F and the tails T */
#define PHT_CD_WORK(n, nh) ((size_t)(3 + (n) + (nh)) * (PHT_LLU_MAXK + 1))

/* words per draw, and where they are */
PHT_HD int pht_cd_nwords(int n, int nh) { return n + nh + 3; }
PHT_HD int pht_cd_w_L(int n) { return n; }
PHT_HD int pht_cd_w_D(int n, int j) { return n + 1 + j; }
PHT_HD int pht_cd_w_nbad(int n, int nh) { return n + nh + 1; }
PHT_HD int pht_cd_w_nunits(int n, int nh) { return n + nh + 2; }

/* nh = 0, or the forecast's rule for 1 .. 16 horizons */
PHT_HD int pht_cd_horizons_ok(int nh, const double *h) {
  if (nh == 0) return 1;
  return (nh <= PHT_CD_MAXH) && pht_fc_horizons_ok(nh, h);
}

/* the a-priori bound on |phi^_j - phi_j| (phi: the truth) */
PHT_HD double pht_cd_phi_bound(int n, int khi, double phi) {
  return (0x1p-53 * (2.0 * (double)(n + 9) * (double)(khi + 1) + (double)(n + 2))) * phi + 0x1p-56;
}

/* the recorded relative bound of r_h at lam = mu h */
PHT_HD double pht_cd_r_bound(double lam) { return PHT_CD_R_R * (lam + 8.0); }

/* F[k n + j] = f_k[j], k = 0..K (S column-major, n <= 32).  The kernel runs the
 * same recurrence with column j in lane j. */
PHT_HD void pht_cd_forward(int n, const double *S, double mu, int K, double *F) {
  double R[32 * 32], fn[32];
  const double rinv = 1.0 / mu;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) R[i * n + j] = pht_llu_R(S[i + j * n], rinv, i == j);
  for (int j = 0; j < n; j++) F[j] = (j == 0) ? 1.0 : 0.0;
  for (int k = 1; k <= K; k++) {
    const double *f = F + (size_t)(k - 1) * n;
    for (int j = 0; j < n; j++) {
      double v = 0.0;
      for (int l = 0; l < n; l++) v = fma(f[l], R[l * n + j], v);
      fn[j] = v;
    }
    for (int j = 0; j < n; j++) F[(size_t)k * n + j] = fn[j];
  }
}

/* m = (-S)^-1 1 (S column-major; its diagonal is not read).  Returns 0 or
 * PHT_CD_F_TRAP (m is then not to be used). */
PHT_HD unsigned pht_cd_mean(int n, const double *S, const double *s, double *m) {
  double A[32 * 32], e[32], b[32], d[32];
  unsigned flag = 0;
  for (int i = 0; i < n; i++) {
    for (int j = 0; j < n; j++) A[i * n + j] = S[i + j * n];
    e[i] = s[i];
    b[i] = 1.0;
  }
  for (int k = n - 1; k >= 0; k--) {
    double dk = e[k];
    for (int j = 0; j < k; j++) dk = dk + A[k * n + j];
    d[k] = dk;
    if (!((dk > 0.0) && (dk < INFINITY))) flag |= PHT_CD_F_TRAP;
    for (int i = 0; i < k; i++) {
      const double t = A[i * n + k] / dk;
      for (int j = 0; j < k; j++)
        if (j != i) A[i * n + j] = fma(t, A[k * n + j], A[i * n + j]);
      e[i] = fma(t, e[k], e[i]);
      b[i] = fma(t, b[k], b[i]);
    }
  }
  for (int k = 0; k < n; k++) {
    double v = b[k];
    for (int j = 0; j < k; j++) v = fma(A[k * n + j], m[j], v);
    m[k] = v / d[k];
  }
  return flag;
}

/* r[j n + i] = r_{h_j}[i], j = 0..nh-1 (nh >= 1, the horizons ok).  T: room for
 * nh (PHT_LLU_MAXK + 1) doubles.  Returns 0 or PHT_CD_F_HCAP (r untouched). */
PHT_HD unsigned pht_cd_renewal(int n, const double *S, const double *s, double mu, int nh, const double *h, double *T,
                               double *r) {
  const int Kr = pht_llu_K(mu, h[nh - 1]);
  if (Kr >= PHT_LLU_MAXK) return PHT_CD_F_HCAP;
  const double rinv = 1.0 / mu;
  const int rows = Kr + 1;
  for (int j = 0; j < nh; j++) {
    double *w = T + (size_t)j * rows;
    const double lam = mu * h[j];
    const int k0 = (lam < (double)Kr) ? (int)floor(lam) : Kr;
    const double il = 1.0 / lam;
    double den = 1.0, x = 1.0;
    w[k0] = 1.0;
    for (int k = k0; k > 0;) {
      x = x * ((double)k * il);
      k--;
      w[k] = x;
      den = den + x;
    }
    x = 1.0;
    for (int k = k0; k < Kr;) {
      k++;
      x = x * (lam * (1.0 / (double)k));
      w[k] = x;
      den = den + x;
    }
    double acc = 0.0;
    for (int k = Kr; k >= 0; k--) {
      const double wk = w[k];
      w[k] = acc / den;
      acc = acc + wk;
    }
  }
  double P[32 * 32], u[32], un[32];
  for (int i = 0; i < n; i++) {
    for (int j = 0; j < n; j++) P[i * n + j] = pht_llu_R(S[i + j * n], rinv, i == j);
    P[i * n] = P[i * n] + s[i] * rinv;
    u[i] = s[i];
  }
  for (int j = 0; j < nh * n; j++) r[j] = 0.0;
  for (int k = 0; k <= Kr; k++) {
    if (k) {
      for (int i = 0; i < n; i++) {
        double v = 0.0;
        for (int j = 0; j < n; j++) v = fma(P[i * n + j], u[j], v);
        un[i] = v;
      }
      for (int i = 0; i < n; i++) u[i] = un[i];
    }
    for (int j = 0; j < nh; j++) {
      const double t = T[(size_t)j * rows + k];
      for (int i = 0; i < n; i++) r[j * n + i] = fma(t, u[i], r[j * n + i]);
    }
  }
  for (int j = 0; j < nh * n; j++) r[j] = rinv * r[j];
  return 0;
}

/* one usable draw's vectors: m[n], r[nh n], scales[1 + nh] = [mscale,
 * dscale_j].  Returns the two new flags (0: usable). */
PHT_HD unsigned pht_cd_vectors(int n, const double *S, const double *s, double mu, int nh, const double *h, double *T,
                               double *m, double *r, double *scales) {
  unsigned flag = pht_cd_mean(n, S, s, m);
  if (nh > 0) flag |= pht_cd_renewal(n, S, s, mu, nh, h, T, r);
  if (flag) return flag;
  double mx = 0.0;
  for (int j = 0; j < n; j++) mx = (m[j] > mx) ? m[j] : mx;
  scales[0] = pht_es_yscale(mx);
  for (int j = 0; j < nh; j++) {
    mx = 0.0;
    for (int i = 0; i < n; i++) mx = (r[j * n + i] > mx) ? r[j * n + i] : mx;
    scales[1 + j] = pht_es_yscale(mx);
  }
  return 0;
}

/* the second pass over a good unit's window: v[j] = sum_k w_k F[k][j].  nmax:
 * the length of v the caller's loops are written for (a compile-time constant
 * in the kernel, so that v stays in registers; n on the host) */
PHT_HD void pht_cd_phase(const double *F, int n, int nmax, const double *invk, const pht_es_win_t *win, double *v) {
  int k = win->k0;
  const double *f = F + (size_t)k * n;
  PHT_CD_UNROLL
  for (int j = 0; j < nmax; j++)
    if (j < n) v[j] = f[j];
  double w = 1.0;
  while (k > win->klo) {
    w = pht_es_down(w, k, win->il);
    k--;
    f = F + (size_t)k * n;
    PHT_CD_UNROLL
  for (int j = 0; j < nmax; j++)
      if (j < n) v[j] = fma(w, f[j], v[j]);
  }
  w = 1.0;
  k = win->k0;
  while (k < win->khi) {
    k++;
    w = pht_es_up(w, k, win->lam, invk);
    f = F + (size_t)k * n;
    PHT_CD_UNROLL
  for (int j = 0; j < nmax; j++)
      if (j < n) v[j] = fma(w, f[j], v[j]);
  }
}

/* v -> phi in place */
PHT_HD void pht_cd_phi(int n, int nmax, double *v) {
  double tot = v[0];
  PHT_CD_UNROLL
  for (int j = 1; j < nmax; j++)
    if (j < n) tot = tot + v[j];
  PHT_CD_UNROLL
  for (int j = 0; j < nmax; j++)
    if (j < n) v[j] = v[j] / tot;
}

/* sum_j fma(phi_j, x_j, .) */
PHT_HD double pht_cd_dot(int n, int nmax, const double *phi, const double *x) {
  double a = 0.0;
  PHT_CD_UNROLL
  for (int j = 0; j < nmax; j++)
    if (j < n) a = fma(phi[j], x[j], a);
  return a;
}

/* the fixed-point word of a value in [0, 1 + a few ulps] */
PHT_HD long long pht_cd_fixed(double x) { return llrint(x * PHT_CD_SCALE); }
/* that of a value x <= scale (a power of two) */
PHT_HD long long pht_cd_fixed_scaled(double x, double scale) { return llrint((x / scale) * PHT_CD_SCALE); }

/* The whole specification for one draw on the host (no device): ncens units
 * of ages c, nh horizons (pht_cd_horizons_ok), the tables sized for ymax_c.
 * work: PHT_CD_WORK(n, nh) doubles.  words [pht_cd_nwords], scales [1 + nh]:
 * written (zero for a flagged draw).  phisum [ncens][n], mrlsum [ncens], dsum
 * [ncens][nh], cnt [ncens]: UPDATED (the draws of a chain in order: one call
 * each); phi [ncens][n], mrl [ncens], dd [ncens][nh]: written (NaN where bad);
 * each of the seven may be null.  Returns the draw's flag word. */
PHT_HD unsigned pht_cd_draw(int n, const double *S, const double *s, long ncens, const double *c, double ymax_c, int nh,
                            const double *h, double *work, long long *words, double *scales, double *phisum,
                            double *mrlsum, double *dsum, long long *cnt, double *phi, double *mrl, double *dd) {
  double meta[PHT_LLU_META], m[32], r[PHT_CD_MAXH * 32], v[32];
  double *tab = work, *invk = tab + 2 * (PHT_LLU_MAXK + 1), *F = invk + (PHT_LLU_MAXK + 1);
  double *T = F + (size_t)n * (PHT_LLU_MAXK + 1);
  const int nw = pht_cd_nwords(n, nh);
  unsigned flag = pht_llu_meta(n, S, s, ymax_c, meta);
  for (int j = 0; j < nw; j++) words[j] = 0;
  for (int j = 0; j <= nh; j++) scales[j] = 0.0;
  const double mu = meta[PHT_LLU_M_MU], abar = meta[PHT_LLU_M_ABAR];
  if (!flag) flag = pht_cd_vectors(n, S, s, mu, nh, h, T, m, r, scales);
  if (flag) {
    for (int j = 0; j <= nh; j++) scales[j] = 0.0;
    for (long i = 0; i < ncens; i++) {
      if (phi)
        for (int j = 0; j < n; j++) phi[i * n + j] = NAN;
      if (mrl) mrl[i] = NAN;
      if (dd)
        for (int j = 0; j < nh; j++) dd[i * nh + j] = NAN;
    }
    return flag;
  }
  const int K = (int)meta[PHT_LLU_M_K];
  pht_llu_table(n, S, s, mu, K, tab);
  pht_cd_forward(n, S, mu, K, F);
  for (int k = 0; k <= K; k++) invk[k] = k ? 1.0 / (double)k : 0.0;
  for (long i = 0; i < ncens; i++) {
    int bad;
    pht_es_win_t win;
    (void)pht_es_window(tab, invk, K, mu, abar, c[i], 1, &bad, &win);
    if (bad) {
      words[pht_cd_w_nbad(n, nh)] += 1;
      if (phi)
        for (int j = 0; j < n; j++) phi[i * n + j] = NAN;
      if (mrl) mrl[i] = NAN;
      if (dd)
        for (int j = 0; j < nh; j++) dd[i * nh + j] = NAN;
      continue;
    }
    pht_cd_phase(F, n, n, invk, &win, v);
    pht_cd_phi(n, n, v);
    const double ml = pht_cd_dot(n, n, v, m);
    for (int j = 0; j < n; j++) {
      words[j] += pht_cd_fixed(v[j]);
      if (phisum) phisum[i * n + j] = phisum[i * n + j] + v[j];
      if (phi) phi[i * n + j] = v[j];
    }
    words[pht_cd_w_L(n)] += pht_cd_fixed_scaled(ml, scales[0]);
    if (mrlsum) mrlsum[i] = mrlsum[i] + ml;
    if (mrl) mrl[i] = ml;
    for (int j = 0; j < nh; j++) {
      const double dv = pht_cd_dot(n, n, v, r + j * n);
      words[pht_cd_w_D(n, j)] += pht_cd_fixed_scaled(dv, scales[1 + j]);
      if (dsum) dsum[i * nh + j] = dsum[i * nh + j] + dv;
      if (dd) dd[i * nh + j] = dv;
    }
    words[pht_cd_w_nunits(n, nh)] += 1;
    if (cnt) cnt[i] += 1;
  }
  return flag;
}

#endif /* PHT_CONDITION_H */
