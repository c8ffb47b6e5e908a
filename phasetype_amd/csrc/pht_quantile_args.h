/*
 * pht_quantile_args.h — host/device interface of the quantile kernel
 * (pht_quantile.hip; specification: include/pht_quantile.h).  The draws' meta
 * words and tables are pht_loglik_unif_args.h's (pht_launch_llunif_table).
 */
#ifndef PHT_QUANTILE_ARGS_H
#define PHT_QUANTILE_ARGS_H

#include <hip/hip_runtime.h>

#include "pht_loglik_args.h" /* kLoglikBatch */

namespace pht {

constexpr int kQuantBlock = 256;  /* lanes of a block */
constexpr int kQuantRows = 2048;  /* PHT_LLU_MAXK + 1: rows of a table at the cap */
constexpr int kQuantPoolMax = 4;  /* tables at the cap in the larger of the two LDS pools */

struct QuantileArgs {
  int nd;              /* draws of this launch (1..kLoglikBatch) */
  int np;              /* probabilities */
  int Kmax;            /* the largest K among the draws: a table's LDS slot is 2 (Kmax + 1) doubles */
  int dpb;             /* draws per block (pht_quantile_pack) */
  int lp;              /* lanes per draw: min(np, kQuantBlock) */
  const double *meta;  /* [nd][PHT_LLU_META] */
  const double *thi;   /* [nd] the draws' horizons */
  const double *tab;   /* [nd][stride], written by llunif_table_kernel */
  int stride;
  const double *probs; /* [np], sorted ascending (NaN last) */
  double t0;
  double *t, *lo, *hi; /* [nd][np] each, in the order of probs */
  int *nev;            /* [nd][np] */
  unsigned *flags;     /* [nd][np] */
};

}  // namespace pht

/* The packing rule: a draw takes lp = min(np, 256) lanes, so 256 / lp draws
 * would fill a block's lanes; as many of them as have their table slots
 * (2 (Kmax + 1) doubles each) in the pool are taken, at least one.  The pool
 * holds one table at the cap (*pool = 1: 60 KB of LDS a block, two blocks a
 * CU) unless four hold more draws (*pool = 4: 156 KB, one block a CU).
 * Returns the draws per block. */
extern "C" int pht_quantile_pack(int nd, int np, int Kmax, int *pool);
extern "C" hipError_t pht_launch_quantile(const pht::QuantileArgs *a, hipStream_t st);

#endif
