/*
 * quantile_spec.c — CPU restatement of include/pht_quantile.h over plain
 * arrays: the bit-level checker of the quantile kernel (tests/quantile_ref.py
 * compiles it with -ffp-contract=off into a shared object; no main).  The
 * draw's meta words, table and evaluator are include/pht_loglik_unif.h's.
 */
#include <stdlib.h>

#include "pht_quantile.h"

double qspec_lambda(void) { return PHT_Q_LAMBDA; }
int qspec_maxit(void) { return PHT_Q_MAXIT; }
double qspec_rtol(void) { return PHT_Q_RTOL; }
int qspec_stop(double a, double b) { return pht_q_stop(a, b); }

/* L = log(1 - p) + lS(t0), the header's operations */
double qspec_L(double p, double ls0) { return pht_psis_log1p(-p) + ls0; }

/* the draw's meta words [flag, mu, abar_x, K] and its horizon */
unsigned qspec_meta(int n, const double *S, const double *s, double tmax, double *meta, double *thi) {
  return pht_q_meta(n, S, s, tmax, meta, thi);
}

/* np roots of one draw; returns the draw's flag word */
unsigned qspec_draw(int n, const double *S, const double *s, int np, const double *probs, double t0, double tmax,
                    double *t, double *lo, double *hi, int *nev, unsigned *flags) {
  double *tab = (double *)malloc(sizeof(double) * 3 * (PHT_LLU_MAXK + 1));
  const unsigned flag = pht_q_draw(n, S, s, np, probs, t0, tmax, tab, tab + 2 * (PHT_LLU_MAXK + 1), t, lo, hi, nev,
                                   flags);
  free(tab);
  return flag;
}
