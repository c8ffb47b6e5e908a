/*
 * pht_estep_args.h — host/device interface of the E-step kernels
 * (pht_estep.hip; specification: include/pht_estep.h).  The draws' meta words
 * and tables are pht_loglik_unif_args.h's (pht_launch_llunif_table).
 */
#ifndef PHT_ESTEP_ARGS_H
#define PHT_ESTEP_ARGS_H

#include <hip/hip_runtime.h>

#include "pht_loglik_args.h" /* kLoglikBatch */

namespace pht {

struct EstepHistArgs {
  int nd;                     /* draws of this launch (1..kLoglikBatch) */
  int Kmax;                   /* the largest K among them */
  long count;                 /* observations of the shard */
  const double *y;            /* [count], the context's (sorted) order */
  const int *cens;            /* [count] */
  const double *meta;         /* [nd][PHT_LLU_META] */
  const double *tab;          /* [nd][stride], written by llunif_table_kernel */
  int stride;
  double ryscale;             /* 1 / yscale */
  unsigned long long *totals; /* [nd][4] int64 [H, F, nbad, nobs], accumulated */
  unsigned long long *words;  /* [nd][PHT_ES_WORDS] int64 [class][k][G, T], accumulated */
};

struct EstepContractArgs {
  int n;
  int nd;                  /* draws of this launch, one workgroup each */
  const double *S;         /* [nd][n * n] column-major generators */
  const double *s;         /* [nd][n] */
  const double *meta;      /* [nd][PHT_LLU_META] */
  const double *tab;       /* [nd][stride] */
  int stride;
  const long long *words;  /* [nd][PHT_ES_WORDS], complete (all shards summed) */
  double yscale;
  double *out;             /* [nd][n * n + 3 n]: Z[n], N[n n] (N[i + j n]), E[n], A[n] */
};

}  // namespace pht

/* grid_cap: most blocks to launch (each takes tiles of 1024 observations) */
extern "C" hipError_t pht_launch_estep_hist(const pht::EstepHistArgs *a, int grid_cap, hipStream_t st);
extern "C" hipError_t pht_launch_estep_contract(const pht::EstepContractArgs *a, hipStream_t st);

#endif
