/*
 * pht_predict_args.h — host/device interface of the posterior-predictive
 * kernel (pht_predict.hip; specification: include/pht_predict.h).
 */
#ifndef PHT_PREDICT_ARGS_H
#define PHT_PREDICT_ARGS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pht {

constexpr int kPpredBatch = 64;  /* most draws of one launch */
constexpr int kPpredBlock = 256; /* lanes of a block */

struct PpredArgs {
  int n;
  int nd;                     /* draws of this launch (1..kPpredBatch): blockIdx.y */
  uint32_t nrep;              /* replicates per draw (1..2^22) */
  uint32_t rep0, draw0;       /* stream numbers of replicate 0 and of this launch's draw 0 */
  uint32_t k0, k1;            /* the Philox key of the launch */
  double horizon;             /* +inf: none */
  int max_jumps;              /* 1..kMaxJumps */
  int ne;                     /* edges (0..1024) */
  const int *flags;           /* [nd] non-zero: the draw is skipped */
  const double *tab;          /* [nd][n + n n] (pht_pred_table) */
  const double *edges;        /* [ne] */
  unsigned long long *words;  /* [nd][8] int64 sums, accumulated */
  unsigned long long *ymin;   /* [nd] bit patterns, combined by min (initialised to +inf's) */
  unsigned long long *ymax;   /* [nd] bit patterns, combined by max (initialised to 0) */
  unsigned long long *counts; /* [nd][ne + 1], accumulated */
  double *y;                  /* pointwise mode: [nd][nrep]; else nullptr */
  int *nj;                    /* pointwise mode: [nd][nrep] jumps */
};

}  // namespace pht

/* blocks_per_draw: blocks that share a draw's replicates (each lane takes a
 * static stripe of them) */
extern "C" hipError_t pht_launch_ppred(const pht::PpredArgs *a, int blocks_per_draw, hipStream_t st);

#endif
