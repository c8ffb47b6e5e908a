/*
 * pht_replace_args.h — host/device interface of the age-replacement kernels
 * (pht_replace.hip; specification: include/pht_replace.h).  The draws' meta
 * words and tables are pht_loglik_unif_args.h's (pht_launch_llunif_table).
 */
#ifndef PHT_REPLACE_ARGS_H
#define PHT_REPLACE_ARGS_H

#include <hip/hip_runtime.h>

#include "pht_loglik_args.h" /* kLoglikBatch */

namespace pht {

constexpr int kRpBlock = 256;  /* lanes of a block, of either kernel */
constexpr int kRpRows = 2048;  /* PHT_LLU_MAXK + 1: rows of a table at the cap */
constexpr int kRpWaves = kRpBlock / 64; /* cost pairs a block of the policy kernel takes */

struct ReplaceCurveArgs {
  int nd;              /* draws of this launch (1..kLoglikBatch) */
  int G;               /* ages */
  int Kmax;            /* the largest K among the draws: an LDS slot is 3 (Kmax + 1) doubles */
  int dpb;             /* draws per block (pht_replace_pack) */
  int lp;              /* lanes per draw: min(G, kRpBlock) */
  const double *meta;  /* [nd][PHT_LLU_META] */
  const double *thi;   /* [nd] the draws' horizons */
  const double *tab;   /* [nd][stride], written by llunif_table_kernel */
  int stride;
  const double *ages;  /* [G] */
  double *cc;          /* [nd][ccstride]: the draws' prefix sums, written (the policy kernel reads them) */
  int ccstride;        /* >= Kmax + 1 */
  double *lS, *lf, *M; /* [nd][G] each */
  unsigned *aflags;    /* [nd][G] */
};

struct ReplacePolicyArgs {
  int nd, G, P, Kmax;
  const double *meta;  /* [nd][PHT_LLU_META] */
  const double *mean;  /* [nd] m = E[T] */
  const double *tab;   /* [nd][stride] */
  int stride;
  const double *cc;    /* [nd][ccstride], written by the curve kernel */
  int ccstride;
  const double *ages;  /* [G] */
  const double *lS, *lf, *M; /* [nd][G], written by the curve kernel */
  const unsigned *aflags;
  const double *cp, *cf;     /* [P] */
  double *t, *g, *lo, *hi;   /* [nd][P] each */
  int *j, *nev;              /* [nd][P] */
  unsigned *flags;           /* [nd][P] */
};

}  // namespace pht

/* The curve kernel's packing rule: a draw takes lp = min(G, 256) lanes, so
 * 256 / lp draws would fill a block's lanes; as many of them as have their
 * slots (3 (Kmax + 1) doubles each: table and prefix sums) in the pool of one
 * slot at the cap are taken, at least one.  Returns the draws per block. */
extern "C" int pht_replace_pack(int nd, int G, int Kmax);
extern "C" hipError_t pht_launch_replace_curve(const pht::ReplaceCurveArgs *a, hipStream_t st);
extern "C" hipError_t pht_launch_replace_policy(const pht::ReplacePolicyArgs *a, hipStream_t st);

#endif
