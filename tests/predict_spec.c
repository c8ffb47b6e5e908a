/*
 * predict_spec.c — CPU restatement of include/pht_predict.h over plain arrays:
 * the bit-level checker of the posterior-predictive kernel
 * (tests/predict_ref.py compiles it with -ffp-contract=off into a shared
 * object; no main).  One draw per call, its replicates one after another.
 */
#include <stdint.h>
#include <string.h>

#include "pht_predict.h"

int pspec_tab_words(int n) { return pht_pred_tab_words(n); }

unsigned pspec_flags(int n, const double *S, const double *s) { return pht_pred_flags(n, S, s); }

void pspec_table(int n, const double *S, const double *s, double *tab) { pht_pred_table(n, S, s, tab); }

/* replicates rep0 .. rep0 + nrep - 1 of draw number `draw` from its table:
 * y[r] (NaN: bad), nj[r], the 8 int64 words, counts[ne + 1], *ymin / *ymax
 * (+inf / -inf when nothing was recorded) */
void pspec_run(int n, const double *tab, uint32_t k0, uint32_t k1, uint32_t rep0, long nrep, uint32_t draw,
               double horizon, int max_jumps, int ne, const double *edges, double *y, int *nj, long long *words,
               long long *counts, double *ymin, double *ymax) {
  uint64_t lo = pht_d2u(INFINITY), hi = 0;
  memset(words, 0, sizeof(long long) * PHT_PRED_WORDS);
  memset(counts, 0, sizeof(long long) * (size_t)(ne + 1));
  for (long r = 0; r < nrep; r++) {
    int oc = 0;
    y[r] = pht_pred_path(n, tab, k0, k1, rep0 + (uint32_t)r, draw, horizon, max_jumps, &nj[r], &oc);
    if (oc & PHT_PRED_BAD) {
      words[PHT_PRED_W_NBAD] += 1;
      continue;
    }
    long long h, f;
    pht_ll_fixed(y[r], &h, &f);
    words[PHT_PRED_W_HY] += h;
    words[PHT_PRED_W_FY] += f;
    pht_ll_fixed(y[r] * y[r], &h, &f);
    words[PHT_PRED_W_HQ] += h;
    words[PHT_PRED_W_FQ] += f;
    words[PHT_PRED_W_NDONE] += 1;
    words[PHT_PRED_W_NSURV] += (oc & PHT_PRED_SURV) ? 1 : 0;
    words[PHT_PRED_W_NJUMP] += nj[r];
    const uint64_t b = pht_d2u(y[r]);
    lo = b < lo ? b : lo;
    hi = b > hi ? b : hi;
    counts[pht_pred_bin(edges, ne, y[r])] += 1;
  }
  *ymin = words[PHT_PRED_W_NDONE] ? pht_u2d(lo) : INFINITY;
  *ymax = words[PHT_PRED_W_NDONE] ? pht_u2d(hi) : -INFINITY;
}
