/*
 * psis_spec.c — the tests' CPU restatement of include/pht_psis.h: the
 * header's own definition (pht_psis_obs) over the observations of a
 * log-likelihood matrix, compiled with cc -O2 -ffp-contract=off
 * (tests/psis_ref.py).
 */
#include <stdlib.h>

#include "pht_psis.h"

int spec_tail_len(int S) { return pht_psis_tail_len(S); }
int spec_grid(int M) { return pht_psis_grid(M); }
double spec_log1p(double z) { return pht_psis_log1p(z); }
double spec_expm1(double z) { return pht_psis_expm1(z); }

/* l: [S][N] (usable draws only, draw order); outputs [N] each.  Returns 0, or
 * -1 when S is out of range or memory is short. */
int spec_psis(int S, long N, const double *l, double *elpd, double *khat, double *lppd, int *flags) {
  if (S < 1 || S > PHT_PSIS_MAXS || N < 0) return -1;
  double *col = (double *)malloc(sizeof(double) * 3 * (size_t)S);
  if (!col) return -1;
  for (long i = 0; i < N; i++) {
    for (int d = 0; d < S; d++) col[d] = l[(size_t)d * (size_t)N + (size_t)i];
    pht_psis_obs(S, col, col + S, elpd + i, khat + i, lppd + i, flags + i);
  }
  free(col);
  return 0;
}
