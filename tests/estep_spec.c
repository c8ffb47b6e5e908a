/*
 * estep_spec.c — CPU restatement of include/pht_estep.h over plain arrays: the
 * bit-level checker of the E-step kernels (tests/estep_ref.py compiles it with
 * -ffp-contract=off into a shared object; no main).  The draw's meta words and
 * table are tests/loglik_unif_spec.c's.
 */
#include <stdlib.h>

#include "pht_estep.h"

int espec_words(void) { return PHT_ES_WORDS; }
int espec_idx(int cls, int k, int q) { return pht_es_idx(cls, k, q); }
double espec_yscale(double ymax) { return pht_es_yscale(ymax); }

/* one usable draw over `count` observations: words[PHT_ES_WORDS] and
 * totals[4] = [H, F, nbad, nobs] are added to; l (NaN where bad), klo and khi
 * per observation */
void espec_hist(int K, double mu, double abar_x, const double *tab, long count, const double *y, const int *cens,
                double yscale, long long *words, long long *totals, double *l, int *klo, int *khi) {
  double *invk = (double *)malloc(sizeof(double) * (size_t)(K + 1));
  for (int k = 0; k <= K; k++) invk[k] = k ? 1.0 / (double)k : 0.0;
  for (long i = 0; i < count; i++) {
    int bad = 0;
    pht_es_win_t win;
    l[i] = pht_es_window(tab, invk, K, mu, abar_x, y[i], cens[i] != 0, &bad, &win);
    klo[i] = win.klo;
    khi[i] = win.khi;
    if (bad) {
      totals[2] += 1;
      continue;
    }
    long long h, f;
    pht_ll_fixed(l[i], &h, &f);
    totals[0] += h;
    totals[1] += f;
    totals[3] += 1;
    pht_es_obs(tab, invk, &win, y[i], yscale, cens[i] != 0, words);
  }
  free(invk);
}

unsigned espec_contract(int n, const double *S, const double *s, const long long *words, int K, double yscale,
                        double *Z, double *N, double *E, double *A) {
  return pht_es_contract(n, S, s, words, K, yscale, Z, N, E, A);
}
