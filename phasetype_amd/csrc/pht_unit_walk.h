/*
 * pht_unit_walk.h — the walk the unit kernels share (llunif_kernel,
 * fcast_kernel, cond_kernel, spares_kernel): one lane per unit
 * (sorted, so neighbouring lanes walk neighbouring k) in tiles of BLOCK over a
 * capped grid, the launch's draws in passes of as many whole (ax, ac) tables
 * as fit kUnitPool doubles of LDS; invk[k] and the table rows come from LDS in
 * the hot loop.  Lanes past the last unit are masked (live = false), never
 * returned early: every lane meets every barrier and wave shuffle.  The kernel
 * declares the LDS arrays (its static LDS is its own), zeroes its block sums
 * between unit_stage and its own __syncthreads(), and flushes them after
 * unit_walk.  Device only.
 */
#ifndef PHT_UNIT_WALK_H
#define PHT_UNIT_WALK_H

#include <hip/hip_runtime.h>

#include "pht_loglik_unif.h"
#include "pht_wave.h"

namespace pht {

constexpr int kUnitPool = 2 * (PHT_LLU_MAXK + 1); /* doubles of (ax, ac) table per pass */

/* an unflagged draw of the pass, as the kernel's body takes it */
struct UnitDraw {
  int d, K; /* the draw of the launch; its table's last row, capped at the launch's Kmax */
  double mu, abar;
  const double *tab; /* its (ax_k, ac_k) in LDS */
};

/* the math tables, 1 / k up to Kmax and the launch's meta words into LDS
 * (the caller's barrier follows) */
template <int BLOCK>
__device__ __forceinline__ void unit_stage(double *sinvk, double *smeta, const double *meta, int nd, int Kmax) {
  const int tid = threadIdx.x;
  pht_stage_math_tables();
  for (int k = tid; k <= Kmax; k += BLOCK) sinvk[k] = k ? 1.0 / (double)k : 0.0;
  for (int k = tid; k < nd * PHT_LLU_META; k += BLOCK) smeta[k] = meta[k];
}

/* Pos: the width of a unit's position.  Per tile and lane: open(pos, live)
 * loads the unit's state, then in draw order flagged(d, pos, live) for an
 * unusable draw (it takes no room in the pool) or draw(UnitDraw, pos, live),
 * then close(pos, live) stores the state, once per pass. */
template <int BLOCK, class Pos, class Open, class Flagged, class Draw, class Close>
__device__ __forceinline__ void unit_walk(double *stab, const double *smeta, const double *tab, int stride, int nd,
                                          int Kmax, Pos count, Open open, Flagged flagged, Draw draw, Close close) {
  const int tid = threadIdx.x;
  for (int d0 = 0; d0 < nd;) {
    /* this pass: draws [d0, d1), as many whole tables as fit the pool (the
     * same count in every lane) */
    int d1 = d0, used = 0;
    while (d1 < nd) {
      const double *m = smeta + d1 * PHT_LLU_META;
      const int need = (__double_as_longlong(m[PHT_LLU_M_FLAG]) != 0) ? 0 : 2 * (min((int)m[PHT_LLU_M_K], Kmax) + 1);
      if (used + need > kUnitPool) break;
      for (int k = tid; k < need; k += BLOCK) stab[used + k] = tab[(size_t)d1 * stride + k];
      used += need;
      d1++;
    }
    __syncthreads();

    for (Pos base = (Pos)blockIdx.x * BLOCK; base < count; base += (Pos)gridDim.x * BLOCK) {
      const Pos pos = base + tid;
      const bool live = pos < count;
      open(pos, live);
      int off = 0;
      for (int d = d0; d < d1; d++) {
        const double *m = smeta + d * PHT_LLU_META;
        if (__double_as_longlong(m[PHT_LLU_M_FLAG]) != 0) { /* the same for every lane */
          flagged(d, pos, live);
          continue;
        }
        const int K = min((int)m[PHT_LLU_M_K], Kmax);
        const UnitDraw u = {d, K, m[PHT_LLU_M_MU], m[PHT_LLU_M_ABAR], stab + off};
        off += 2 * (K + 1);
        draw(u, pos, live);
      }
      close(pos, live);
    }
    d0 = d1;
    __syncthreads(); /* every lane is done with this pass's tables */
  }
}

}  // namespace pht

#endif
