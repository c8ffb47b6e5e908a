/*
 * loglik_unif_spec.c — CPU restatement of include/pht_loglik_unif.h over plain
 * arrays: the bit-level checker of the uniformisation log-likelihood kernels
 * (tests/loglik_unif_ref.py compiles it with -ffp-contract=off into a shared
 * object; no main).  Totals and the WAIC recurrence are tests/loglik_spec.c's.
 */
#include <stdlib.h>

#include "pht_loglik_unif.h"

int uspec_K(double mu, double ymax) { return pht_llu_K(mu, ymax); }

/* the draw's meta words [flag, mu, abar_x, K]; returns the flag word */
unsigned uspec_meta(int n, const double *S, const double *s, double ymax, double *meta) {
  return pht_llu_meta(n, S, s, ymax, meta);
}

/* tab[2 k] = ax_k, tab[2 k + 1] = ac_k, k = 0..K, of a usable draw */
void uspec_table(int n, const double *S, const double *s, double mu, int K, double *tab) {
  pht_llu_table(n, S, s, mu, K, tab);
}

/* l[i] (NaN where bad) and the upper window end khi[i] for every observation
 * from one usable draw's table */
void uspec_pointwise(int K, double mu, double abar_x, const double *tab, long count, const double *y, const int *cens,
                     double *l, int *khi) {
  double *invk = (double *)malloc(sizeof(double) * (size_t)(K + 1));
  for (int k = 0; k <= K; k++) invk[k] = k ? 1.0 / (double)k : 0.0;
  for (long i = 0; i < count; i++) {
    int bad = 0;
    l[i] = pht_llu_eval(tab, invk, K, mu, abar_x, y[i], cens[i] != 0, &bad, &khi[i]);
  }
  free(invk);
}
