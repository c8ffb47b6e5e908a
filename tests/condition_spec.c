/*
 * condition_spec.c — CPU restatement of include/pht_condition.h over plain
 * arrays: the bit-level checker of the condition kernels
 * (tests/condition_ref.py compiles it with -ffp-contract=off into a shared
 * object; no main).  The draw's meta words, table and window are
 * include/pht_loglik_unif.h's and include/pht_estep.h's.
 */
#include <stdlib.h>

#include "pht_condition.h"

int cspec_maxh(void) { return PHT_CD_MAXH; }
long cspec_maxunits(void) { return PHT_CD_MAXUNITS; }
double cspec_scale(void) { return PHT_CD_SCALE; }
double cspec_m_r(void) { return PHT_CD_M_R; }
double cspec_r_r(void) { return PHT_CD_R_R; }
double cspec_r_bound(double lam) { return pht_cd_r_bound(lam); }
unsigned cspec_f_trap(void) { return PHT_CD_F_TRAP; }
unsigned cspec_f_hcap(void) { return PHT_CD_F_HCAP; }
int cspec_nwords(int n, int nh) { return pht_cd_nwords(n, nh); }
int cspec_horizons_ok(int nh, const double *h) { return pht_cd_horizons_ok(nh, h); }
double cspec_phi_bound(int n, int khi, double phi) { return pht_cd_phi_bound(n, khi, phi); }

/* m[n]; returns the flag */
unsigned cspec_mean(int n, const double *S, const double *s, double *m) { return pht_cd_mean(n, S, s, m); }

/* r[nh][n] and Kr; returns the flag */
unsigned cspec_renewal(int n, const double *S, const double *s, double mu, int nh, const double *h, double *r,
                       int *Kr) {
  double *T = (double *)malloc(sizeof(double) * (size_t)nh * (PHT_LLU_MAXK + 1));
  const unsigned flag = pht_cd_renewal(n, S, s, mu, nh, h, T, r);
  *Kr = pht_llu_K(mu, h[nh - 1]);
  free(T);
  return flag;
}

/* the windows of the units of one usable draw: l, bad, khi per unit */
void cspec_windows(int n, const double *S, const double *s, long ncens, const double *c, double ymax_c, double *l,
                   int *bad, int *khi) {
  double meta[PHT_LLU_META];
  if (pht_llu_meta(n, S, s, ymax_c, meta)) return;
  const int K = (int)meta[PHT_LLU_M_K];
  double *tab = (double *)malloc(sizeof(double) * 3 * (PHT_LLU_MAXK + 1)), *invk = tab + 2 * (PHT_LLU_MAXK + 1);
  pht_llu_table(n, S, s, meta[PHT_LLU_M_MU], K, tab);
  for (int k = 0; k <= K; k++) invk[k] = k ? 1.0 / (double)k : 0.0;
  for (long i = 0; i < ncens; i++) {
    pht_es_win_t win;
    l[i] = pht_es_window(tab, invk, K, meta[PHT_LLU_M_MU], meta[PHT_LLU_M_ABAR], c[i], 1, bad + i, &win);
    khi[i] = win.khi;
  }
  free(tab);
}

/* one draw: pht_cd_draw (the sums updated; any of the last seven may be null) */
unsigned cspec_draw(int n, const double *S, const double *s, long ncens, const double *c, double ymax_c, int nh,
                    const double *h, long long *words, double *scales, double *phisum, double *mrlsum, double *dsum,
                    long long *cnt, double *phi, double *mrl, double *dd) {
  double *work = (double *)malloc(sizeof(double) * PHT_CD_WORK(n, nh));
  const unsigned flag =
      pht_cd_draw(n, S, s, ncens, c, ymax_c, nh, h, work, words, scales, phisum, mrlsum, dsum, cnt, phi, mrl, dd);
  free(work);
  return flag;
}
