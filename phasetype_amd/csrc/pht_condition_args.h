/*
 * pht_condition_args.h — host/device interface of the condition kernels
 * (pht_condition.hip; specification: include/pht_condition.h).  The draws'
 * meta words and (ax, ac) tables are pht_loglik_unif_args.h's
 * (pht_launch_llunif_table); the host ORs the specification's own two flags
 * into a draw's meta flag word, so that every kernel skips the same draws.
 */
#ifndef PHT_CONDITION_ARGS_H
#define PHT_CONDITION_ARGS_H

#include <hip/hip_runtime.h>

#include "pht_loglik_args.h" /* kLoglikBatch */

namespace pht {

constexpr int kCondBlock = 512; /* lanes of a block (= units of a tile) */
constexpr int kCondMaxH = 16;   /* PHT_CD_MAXH */

/* the forward tables of a batch: one wavefront per draw */
struct CondTableArgs {
  int n, nd;
  const double *S;    /* [nd][n n] column-major */
  const double *meta; /* [nd][PHT_LLU_META] */
  double *F;          /* [nd][fstride]: F[k n + j], k = 0 .. min(K, rows - 1) */
  long fstride;       /* doubles per draw, rows n */
  int rows;           /* rows a draw has room for (the largest K of the call + 1) */
};

/* doubles of one draw's vectors: m[n], r[nh][n], scales[1 + nh] */
constexpr int cond_vec_doubles(int n, int nh) { return n + nh * n + 1 + nh; }

struct CondArgs {
  int n;              /* states (1..kMaxN) */
  int nd;             /* draws of this launch (1..kLoglikBatch) */
  int nh;             /* horizons (0..kCondMaxH) */
  int Kmax;           /* the largest K among the draws (invk is staged up to it) */
  long count;         /* censored units of the context */
  const double *age;  /* [count] their ages, the context's (sorted) order */
  const double *meta; /* [nd][PHT_LLU_META] */
  const double *tab;  /* [nd][stride], written by llunif_table_kernel */
  int stride;
  const double *F;    /* [nd][fstride], written by cond_forward_kernel */
  long fstride;
  const double *vec;  /* [nd][cond_vec_doubles(n, nh)], from the host (pht_cd_vectors) */
  unsigned long long *words; /* [nd][n + nh + 3]: all but the last (nunits, the host's) accumulated */
  double *state;      /* [count][n + 2 + nh]: phisum_j, mrlsum, dsum_h and cnt (as a double) of every unit,
                         updated in draw order */
  double *pw;         /* pointwise mode: [count][nd][n + 1 + nh] = (phi, MRL, D), units in the age order; else nullptr */
};

}  // namespace pht

extern "C" hipError_t pht_launch_cond_forward(const pht::CondTableArgs *a, hipStream_t st);
/* grid_cap: most blocks to launch (each takes tiles of kCondBlock units) */
extern "C" hipError_t pht_launch_cond(const pht::CondArgs *a, int grid_cap, hipStream_t st);

#endif
