/*
 * spares_spec.c — CPU restatement of include/pht_spares.h over plain arrays:
 * the bit-level checker of the spares kernels (tests/spares_ref.py compiles it
 * with -ffp-contract=off into a shared object; no main).  The draw's meta
 * words, table, window and phase law are include/pht_loglik_unif.h's,
 * include/pht_estep.h's and include/pht_condition.h's.
 */
#include <stdlib.h>

#include "pht_spares.h"

double sspec_q_r(void) { return PHT_SP_Q_R; }
double sspec_v_r(void) { return PHT_SP_V_R; }
double sspec_q_bound(double lam) { return pht_sp_q_bound(lam); }
double sspec_var_bound(double lam, double D, double Q) { return pht_sp_var_bound(lam, D, Q); }
int sspec_nwords(int nh) { return pht_sp_nwords(nh); }
int sspec_horizons_ok(int nh, const double *h) { return pht_sp_horizons_ok(nh, h); }
double sspec_var(double D, double Q) { return pht_sp_var(D, Q); }

/* r[nh][n], q[nh][n], scales[2 nh] and Kr; returns the specification's own flags (nothing written where set) */
unsigned sspec_vectors(int n, const double *S, const double *s, double mu, int nh, const double *h, double *r,
                       double *q, double *scales, int *Kr) {
  const unsigned flag = pht_sp_flags(n, S, s, mu, h[nh - 1]);
  *Kr = pht_llu_K(mu, h[nh - 1]);
  if (flag) return flag;
  double *W = (double *)malloc(sizeof(double) * PHT_SP_WDOUBLES(nh, *Kr + 1));
  pht_sp_vectors(n, S, s, mu, nh, h, W, r, q, scales);
  free(W);
  return 0;
}

/* one draw: pht_sp_draw (the sums updated; any of the last six may be null) */
unsigned sspec_draw(int n, const double *S, const double *s, long ncens, const double *c, double ymax_c, int nh,
                    const double *h, long long *words, double *scales, double *dsum, double *vsum, double *d2sum,
                    long long *cnt, double *dd, double *var) {
  double *work = (double *)malloc(sizeof(double) * PHT_SP_WORK(n, nh));
  const unsigned flag =
      pht_sp_draw(n, S, s, ncens, c, ymax_c, nh, h, work, words, scales, dsum, vsum, d2sum, cnt, dd, var);
  free(work);
  return flag;
}
