/*
 * pht_psis_args.h — host/device interface of the PSIS-LOO kernels
 * (pht_psis.hip; specification: include/pht_psis.h).
 */
#ifndef PHT_PSIS_ARGS_H
#define PHT_PSIS_ARGS_H

#include <hip/hip_runtime.h>

namespace pht {

/* a chunk of observations of the pointwise matrix [ndraws][count], usable
 * rows only, transposed into [observation][usable draw] */
struct PsisTransposeArgs {
  const double *mat; /* [ndraws][count], the context's (sorted) observation order */
  long count;        /* its leading dimension */
  const int *rows;   /* [S] the usable rows, ascending */
  int S;
  long k0;           /* first observation of the chunk */
  long kc;           /* observations of the chunk */
  double *out;       /* [kc][S] */
};

struct PsisArgs {
  const double *lt; /* [kc][S] (PsisTransposeArgs.out) */
  int S;            /* usable draws, 1..PHT_PSIS_MAXS */
  long kc;
  double *elpd, *khat, *lppd; /* [kc] each */
  int *flags;                 /* [kc] */
};

}  // namespace pht

extern "C" hipError_t pht_launch_psis_transpose(const pht::PsisTransposeArgs *a, hipStream_t st);
/* grid_cap: most blocks to launch (one wavefront each, striding over the chunk) */
extern "C" hipError_t pht_launch_psis(const pht::PsisArgs *a, int grid_cap, hipStream_t st);

#endif
