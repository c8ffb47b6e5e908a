/*
 * loglik_spec.c — CPU restatement of include/pht_loglik.h over plain arrays:
 * the bit-level checker of the log-likelihood kernel (tests/loglik_ref.py
 * compiles it with -ffp-contract=off into a shared object; no main).
 */
#include "pht_loglik.h"

/* l[i] for every observation from one draw block (NaN where bad, the
 * cancellation guard of pht_ll_finish included, and for every observation of
 * a flagged block) */
void spec_pointwise(int n, const double *blk, long count, const double *y, const int *cens, double *l) {
  uint64_t flag;
  memcpy(&flag, blk + PHT_LL_FLAG, 8);
  for (long i = 0; i < count; i++) {
    int bad = 0;
    l[i] = flag ? NAN : pht_ll_eval(n, blk, y[i], cens[i] != 0, &bad);
  }
}

/* the totals words [H, F, nbad, nobs] of one usable draw from its l values */
void spec_totals(long count, const double *l, long long *tot) {
  tot[0] = tot[1] = tot[2] = tot[3] = 0;
  for (long i = 0; i < count; i++) {
    if (l[i] != l[i]) {
      tot[2] += 1;
      continue;
    }
    long long h, f;
    pht_ll_fixed(l[i], &h, &f);
    tot[0] += h;
    tot[1] += f;
    tot[3] += 1;
  }
}

/* the WAIC recurrence over draws d = 0..ndraws-1 (l[d * count + i]; NaN is
 * skipped), updating the state arrays in place */
void spec_waic(long count, int ndraws, const double *l, double *ref, double *S1, double *S2, double *m, double *r,
               int *cnt) {
  for (long i = 0; i < count; i++) {
    pht_waic_t w = {ref[i], S1[i], S2[i], m[i], r[i], cnt[i]};
    for (int d = 0; d < ndraws; d++) {
      const double v = l[(size_t)d * count + i];
      if (v == v) pht_waic_update(&w, v);
    }
    ref[i] = w.ref;
    S1[i] = w.S1;
    S2[i] = w.S2;
    m[i] = w.m;
    r[i] = w.r;
    cnt[i] = (int)w.cnt;
  }
}
