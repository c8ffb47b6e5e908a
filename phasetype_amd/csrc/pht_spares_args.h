/*
 * pht_spares_args.h — host/device interface of the spares kernels
 * (pht_spares.hip; specification: include/pht_spares.h).  The draws' meta
 * words and (ax, ac) tables are pht_loglik_unif_args.h's
 * (pht_launch_llunif_table) and the forward tables pht_condition_args.h's
 * (pht_launch_cond_forward); the host ORs the specification's two flags into a
 * draw's meta flag word, so that every kernel skips the same draws.
 */
#ifndef PHT_SPARES_ARGS_H
#define PHT_SPARES_ARGS_H

#include <hip/hip_runtime.h>

#include "pht_loglik_args.h" /* kLoglikBatch */

namespace pht {

constexpr int kSparesBlock = 512; /* lanes of a block (= units of a tile) */
constexpr int kSparesMaxH = 16;   /* PHT_CD_MAXH */

/* doubles of one draw's vectors: r[nh][n], q[nh][n], dscale[nh], vscale[nh] */
constexpr int spares_vec_doubles(int n, int nh) { return 2 * nh * n + 2 * nh; }

/* the moment vectors of a batch: one wavefront per draw */
struct SparesVecArgs {
  int n, nd, nh;
  const double *S;    /* [nd][n n] column-major */
  const double *s;    /* [nd][n] */
  const double *meta; /* [nd][PHT_LLU_META] */
  const double *h;    /* [nh] the horizons */
  const int *kr;      /* [nd] Kr = pht_llu_K(mu, h_max) of a usable draw (< rows) */
  double *W;          /* [nd][wstride]: the weights (T_k, p_k), PHT_SP_W; scratch */
  long wstride;       /* doubles per draw, at least 2 nh rows */
  int rows;           /* rows a draw has room for (the largest Kr of the call + 1) */
  double *vec;        /* [nd][spares_vec_doubles(n, nh)], written for a usable draw */
};

struct SparesArgs {
  int n;              /* states (1..kMaxN) */
  int nd;             /* draws of this launch (1..kLoglikBatch) */
  int nh;             /* horizons (1..kSparesMaxH) */
  int Kmax;           /* the largest K among the draws (invk is staged up to it) */
  long count;         /* censored units of the context */
  const double *age;  /* [count] their ages, the context's (sorted) order */
  const double *meta; /* [nd][PHT_LLU_META] */
  const double *tab;  /* [nd][stride], written by llunif_table_kernel */
  int stride;
  const double *F;    /* [nd][fstride], written by the forward-table kernel */
  long fstride;
  const double *vec;  /* [nd][spares_vec_doubles(n, nh)], written by spares_vectors_kernel */
  unsigned long long *words; /* [nd][2 nh + 2]: all but the last (nunits, the host's) accumulated */
  double *state;      /* [count][3 nh + 1]: dsum_h, vsum_h, d2sum_h and cnt (as a double) of every unit, updated in
                         draw order */
  double *pw;         /* pointwise mode: [count][nd][2 nh] = (D, var), units in the age order; else nullptr */
};

}  // namespace pht

extern "C" hipError_t pht_launch_spares_vectors(const pht::SparesVecArgs *a, hipStream_t st);
/* grid_cap: most blocks to launch (each takes tiles of kSparesBlock units) */
extern "C" hipError_t pht_launch_spares(const pht::SparesArgs *a, int grid_cap, hipStream_t st);

#endif
