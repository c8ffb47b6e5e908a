/*
 * forecast_spec.c — CPU restatement of include/pht_forecast.h over plain
 * arrays: the bit-level checker of the forecast kernel (tests/forecast_ref.py
 * compiles it with -ffp-contract=off into a shared object; no main).  The
 * draw's meta words, table and evaluator are include/pht_loglik_unif.h's.
 */
#include <stdlib.h>

#include "pht_forecast.h"

int fspec_maxh(void) { return PHT_FC_MAXH; }
long fspec_maxunits(void) { return PHT_FC_MAXUNITS; }
double fspec_thresh(void) { return PHT_FC_THRESH; }
double fspec_r(void) { return PHT_FC_R; }
double fspec_scale(void) { return PHT_FC_SCALE; }
int fspec_horizons_ok(int nh, const double *h) { return pht_fc_horizons_ok(nh, h); }

/* pht_fc_q over an array */
void fspec_q(long m, const double *dl, double *q) {
  for (long k = 0; k < m; k++) q[k] = pht_fc_q(dl[k]);
}

/* one draw: pht_fc_draw (qsum and cnt updated; any of qsum, cnt, q may be null) */
unsigned fspec_draw(int n, const double *S, const double *s, long ncens, const double *c, double ymax_c, int nh,
                    const double *h, long long *words, double *qsum, long long *cnt, double *q) {
  double *tab = (double *)malloc(sizeof(double) * 3 * (PHT_LLU_MAXK + 1));
  const unsigned flag =
      pht_fc_draw(n, S, s, ncens, c, ymax_c, nh, h, tab, tab + 2 * (PHT_LLU_MAXK + 1), words, qsum, cnt, q);
  free(tab);
  return flag;
}
