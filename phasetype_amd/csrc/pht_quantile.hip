/*
 * pht_quantile.hip — quantiles and residual-life quantiles of posterior draws
 * (specification: include/pht_quantile.h).  The (ax, ac) tables are
 * pht_loglik_unif.hip's (pht_launch_llunif_table); one kernel of its own per
 * batch of draws.
 *
 * quantile_kernel: one lane per (draw, probability), the whole root search of
 * pht_q_root in that lane.  A block of 256 lanes first stages, for each of its
 * draws, the draw's table (32 KB at the cap K = 2047) and once 1 / k (16 KB)
 * in LDS, then one lane per draw evaluates the draw's start (lS(t0) and the
 * hazard at t0, pht_q_start); after that barrier there is none: the searches
 * diverge freely and every lane writes its own five words.  The host sorts the
 * probabilities, so neighbouring lanes walk neighbouring windows of the table.
 *
 * Packing (pht_quantile_pack): with np >= 256 a block is one tile of 256
 * probabilities of one draw (grid: draws x tiles).  With fewer, a draw takes
 * np lanes and a block takes 256 / np draws, as many as have their tables in
 * the pool: the kernel is built with a pool of one table at the cap
 * (quantile_kernel<1>: 60 KB with 1 / k, the starts and the math tables, two
 * blocks a CU) and of four (quantile_kernel<4>: 156 KB, one block a CU, four
 * draws in flight per CU against two).  A smaller K (a finite tmax) packs
 * more draws into either pool.
 */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pht_kernels.h"
#include "pht_layout.h"
#include "pht_loglik_unif_args.h"
#include "pht_quantile.h"
#include "pht_quantile_args.h"

namespace pht {

static_assert(kQuantRows == PHT_LLU_MAXK + 1, "a table at the cap");
static_assert(kQuantBlock % 64 == 0 && kQuantBlock >= 64 && kQuantBlock <= 1024, "whole waves");

template <int G>
__global__ void __launch_bounds__(kQuantBlock) quantile_kernel(const QuantileArgs a) {
  __shared__ double stab[G * 2 * kQuantRows];
  __shared__ double sinvk[kQuantRows];
  __shared__ double sls0[kQuantBlock], shz0[kQuantBlock];
  __shared__ int sbad0[kQuantBlock];
  const int tid = threadIdx.x;
  const int slot = 2 * (a.Kmax + 1);
  const int dbase = blockIdx.x * a.dpb;
  pht_stage_math_tables();
  for (int k = tid; k <= a.Kmax; k += kQuantBlock) sinvk[k] = k ? 1.0 / (double)k : 0.0;
  for (int g = 0; g < a.dpb && dbase + g < a.nd; g++) {
    const int d = dbase + g;
    const double *m = a.meta + (size_t)d * PHT_LLU_META;
    if (__double_as_longlong(m[PHT_LLU_M_FLAG]) != 0) continue; /* flagged draw: no table */
    const int K = min((int)m[PHT_LLU_M_K], a.Kmax);
    for (int k = tid; k < 2 * (K + 1); k += kQuantBlock) stab[g * slot + k] = a.tab[(size_t)d * a.stride + k];
  }
  __syncthreads();
  if (tid < a.dpb && dbase + tid < a.nd) { /* the draw's start, once per draw */
    const double *m = a.meta + (size_t)(dbase + tid) * PHT_LLU_META;
    double ls0 = 0.0, hz0 = 0.0;
    int bad0 = 0;
    if (__double_as_longlong(m[PHT_LLU_M_FLAG]) == 0)
      ls0 = pht_q_start(stab + tid * slot, sinvk, min((int)m[PHT_LLU_M_K], a.Kmax), m[PHT_LLU_M_MU],
                        m[PHT_LLU_M_ABAR], a.thi[dbase + tid], a.t0, &bad0, &hz0);
    sls0[tid] = ls0;
    shz0[tid] = hz0;
    sbad0[tid] = bad0;
  }
  __syncthreads();

  const int g = tid / a.lp, j = tid - g * a.lp;
  const int d = dbase + g;
  const long pi = (long)blockIdx.y * kQuantBlock + j;
  if (g >= a.dpb || d >= a.nd || pi >= (long)a.np) return; /* no barrier below */
  const double *m = a.meta + (size_t)d * PHT_LLU_META;
  pht_q_out_t o;
  if (__double_as_longlong(m[PHT_LLU_M_FLAG]) != 0)
    pht_q_flagged(&o);
  else
    pht_q_root(stab + g * slot, sinvk, min((int)m[PHT_LLU_M_K], a.Kmax), m[PHT_LLU_M_MU], m[PHT_LLU_M_ABAR], a.thi[d],
               a.t0, sls0[g], sbad0[g], shz0[g], a.probs[pi], &o);
  const size_t at = (size_t)d * (size_t)a.np + (size_t)pi;
  a.t[at] = o.t;
  a.lo[at] = o.a;
  a.hi[at] = o.b;
  a.nev[at] = o.nev;
  a.flags[at] = o.flags;
}

}  // namespace pht

extern "C" int pht_quantile_pack(int nd, int np, int Kmax, int *pool) {
  using namespace pht;
  const int lp = np < kQuantBlock ? np : kQuantBlock, slot = 2 * (Kmax + 1);
  const int want = std::min(kQuantBlock / lp, nd);
  const int fit1 = (2 * kQuantRows) / slot, fit4 = (kQuantPoolMax * 2 * kQuantRows) / slot;
  const int d1 = std::max(1, std::min(want, fit1)), d4 = std::max(1, std::min(want, fit4));
  *pool = (d4 > d1) ? kQuantPoolMax : 1;
  return (d4 > d1) ? d4 : d1;
}

extern "C" hipError_t pht_launch_quantile(const pht::QuantileArgs *a, hipStream_t st) {
  using namespace pht;
  if (!a || a->nd < 1 || a->nd > kLoglikBatch || a->np < 1 || !a->meta || !a->thi || !a->tab || !a->probs || !a->t ||
      !a->lo || !a->hi || !a->nev || !a->flags || a->Kmax < 0 || a->Kmax > PHT_LLU_MAXK ||
      a->stride < 2 * (a->Kmax + 1))
    return hipErrorInvalidValue;
  int pool = 1;
  const int dpb = pht_quantile_pack(a->nd, a->np, a->Kmax, &pool);
  /* the launch's packing must be the rule's: the LDS slots are sized by it */
  if (a->dpb != dpb || a->lp != (a->np < kQuantBlock ? a->np : kQuantBlock)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a->nd + dpb - 1) / dpb), (unsigned)((a->np + kQuantBlock - 1) / kQuantBlock));
  if (dpb > 1 && grid.y != 1) return hipErrorInvalidValue;
  if (pool == 1)
    hipLaunchKernelGGL((quantile_kernel<1>), grid, dim3(kQuantBlock), 0, st, *a);
  else
    hipLaunchKernelGGL((quantile_kernel<kQuantPoolMax>), grid, dim3(kQuantBlock), 0, st, *a);
  return hipGetLastError();
}
