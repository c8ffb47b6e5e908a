/*
 * pht_loglik_unif_args.h — host/device interface of the uniformisation
 * log-likelihood kernels (pht_loglik_unif.hip; specification:
 * include/pht_loglik_unif.h).
 */
#ifndef PHT_LOGLIK_UNIF_ARGS_H
#define PHT_LOGLIK_UNIF_ARGS_H

#include <hip/hip_runtime.h>

#include "pht_loglik_args.h" /* kLoglikBatch */

namespace pht {

struct LlunifTableArgs {
  int n;
  int nd;             /* draws of this launch (1..kLoglikBatch), one wavefront each */
  const double *S;    /* [nd][n * n] column-major generators */
  const double *s;    /* [nd][n] exit rates */
  const double *meta; /* [nd][PHT_LLU_META] words [flag, mu, abar_x, K] (pht_llu_meta) */
  double *tab;        /* [nd][stride]: (ax_k, ac_k) interleaved, k = 0..K of the draw */
  int stride;         /* doubles per draw, >= 2 (K + 1) of every draw of the launch */
};

struct LlunifArgs {
  int nd;                      /* draws of this launch (1..kLoglikBatch) */
  int Kmax;                    /* the largest K among them (invk is staged up to it) */
  long count;                  /* observations of the shard */
  const double *y;             /* [count], the context's (sorted) order */
  const int *cens;             /* [count] */
  const double *meta;          /* [nd][PHT_LLU_META] */
  const double *tab;           /* [nd][stride], written by llunif_table_kernel */
  int stride;
  unsigned long long *totals;  /* [nd][4] int64 [H, F, nbad, nobs], accumulated */
  double *pw;                  /* pointwise mode: [nd][count] in the y order; else nullptr */
  int acc;                     /* update the WAIC state below */
  double *w_ref, *w_S1, *w_S2, *w_m, *w_r; /* [count] each */
  long long *w_cnt;            /* [count] */
};

}  // namespace pht

extern "C" hipError_t pht_launch_llunif_table(const pht::LlunifTableArgs *a, hipStream_t st);
/* grid_cap: most blocks to launch (each takes tiles of 512 observations) */
extern "C" hipError_t pht_launch_llunif(const pht::LlunifArgs *a, int grid_cap, hipStream_t st);

#endif
