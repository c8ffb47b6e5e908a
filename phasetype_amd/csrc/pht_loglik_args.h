/*
 * pht_loglik_args.h — host/device interface of the log-likelihood kernel
 * (pht_loglik.hip; specification: include/pht_loglik.h).
 */
#ifndef PHT_LOGLIK_ARGS_H
#define PHT_LOGLIK_ARGS_H

#include <hip/hip_runtime.h>

namespace pht {

constexpr int kLoglikBatch = 64; /* draw blocks staged in LDS per launch */

struct LoglikArgs {
  int n;
  int nd;                      /* draws of this launch (1..kLoglikBatch) */
  long count;                  /* observations of the shard */
  const double *y;             /* [count], the context's (sorted) order */
  const int *cens;             /* [count] */
  const double *blocks;        /* [nd][pht_ll_words(n)] 64-bit words */
  unsigned long long *totals;  /* [nd][4] int64 [H, F, nbad, nobs], accumulated */
  double *pw;                  /* pointwise mode: [nd][count] in the y order; else nullptr */
  int acc;                     /* update the WAIC state below */
  double *w_ref, *w_S1, *w_S2, *w_m, *w_r; /* [count] each */
  long long *w_cnt;            /* [count] */
};

}  // namespace pht

/* grid_cap: most blocks to launch (each takes tiles of 256 observations) */
extern "C" hipError_t pht_launch_loglik(const pht::LoglikArgs *a, int grid_cap, hipStream_t st);

#endif
