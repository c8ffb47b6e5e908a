/*
 * pht_forecast_args.h — host/device interface of the forecast kernel
 * (pht_forecast.hip; specification: include/pht_forecast.h).  The draws' meta
 * words and tables are pht_loglik_unif_args.h's (pht_launch_llunif_table).
 */
#ifndef PHT_FORECAST_ARGS_H
#define PHT_FORECAST_ARGS_H

#include <hip/hip_runtime.h>

#include "pht_loglik_args.h" /* kLoglikBatch */

namespace pht {

constexpr int kFcastBlock = 512; /* lanes of a block (= units of a tile) */
constexpr int kFcastMaxH = 16;   /* PHT_FC_MAXH */
constexpr int kFcastFewH = 4;    /* up to this many horizons: the kernel built with 4 state slots a unit */

struct FcastArgs {
  int nd;             /* draws of this launch (1..kLoglikBatch) */
  int nh;             /* horizons (1..kFcastMaxH) */
  int Kmax;           /* the largest K among the draws (invk is staged up to it) */
  long count;         /* censored units of the context */
  const double *age;  /* [count] their ages, the context's (sorted) order */
  const double *meta; /* [nd][PHT_LLU_META] */
  const double *tab;  /* [nd][stride], written by llunif_table_kernel */
  int stride;
  const double *h;           /* [nh] the horizons, ascending */
  unsigned long long *words; /* [nd][nh][4]: [M, V, nbad] accumulated; word 3 (nunits) is the host's */
  double *qsum;              /* [count][pht_fcast_slots(nh)], updated in draw order (slots past nh stay 0) */
  int *cnt;                  /* [count][pht_fcast_slots(nh)], updated */
  double *q;                 /* pointwise mode: [nd][count][nh] in the age order; else nullptr */
};

}  // namespace pht

/* state slots a unit for nh horizons: the kernel keeps a unit's qsum and cnt
 * of every slot in registers, so it is built for 4 and for 16 of them */
extern "C" int pht_fcast_slots(int nh);
/* grid_cap: most blocks to launch (each takes tiles of kFcastBlock units) */
extern "C" hipError_t pht_launch_fcast(const pht::FcastArgs *a, int grid_cap, hipStream_t st);

#endif
