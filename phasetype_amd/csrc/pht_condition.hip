/*
 * pht_condition.hip — the fleet condition: for every draw and every censored
 * unit of a shard the posterior law of its phase, its mean residual life and
 * its expected failures with replacement (specification:
 * include/pht_condition.h).  The (ax, ac) tables are pht_loglik_unif.hip's
 * (pht_launch_llunif_table, with the K of the largest age); two kernels of its
 * own per batch of draws.  The draw's vectors m, r_h and its scales come from
 * the host (pht_cd_vectors: n^2 (Kr + 1) operations a draw).
 *
 * cond_forward_kernel: one wavefront per draw, llunif_table_kernel turned
 * round.  Lane j keeps column j of R in registers with f[j]; f_{k-1}[l] reaches
 * every lane by a wave shuffle in increasing l; lane j stores F[k][j].  K
 * dependent steps.  The table stays in global memory: n (K + 1) doubles a draw,
 * 164 KB at n = 10, K = 2047, more than LDS holds.
 *
 * cond_kernel: a unit walk (pht_unit_walk.h) over the context's censored units
 * and their sorted ages.  The FIRST pass over a unit's window (pht_es_window)
 * reads invk[k] and the table rows from LDS.  The SECOND pass reads the rows
 * F[k][.] through the caches: the lanes of a wave are at neighbouring k, so a
 * row is read by many lanes at once.  v[n] lives in registers: the kernel is
 * built for n = 3, 5, 10, 15, 20 and once for a runtime n up to 32 (every loop
 * over the phases unrolled to 32 and masked).  Per draw and word: a
 * wave-shuffle sum, one LDS add per wave, one 64-bit atomic per word at the
 * end of the block (nunits = units - nbad is the host's).  A unit's sums and
 * its count live in global memory, [unit][word], read and written by the
 * owning lane once per draw in which the unit is good: in draw order.
 *
 * LDS at n <= 20: 32 KB of tables, 16 KB of 1 / k, 7 KB of math tables, 2 KB
 * of meta words and 19 KB of block sums (64 draws x 38 words): under 80 KB,
 * two blocks a CU; the runtime-n build has 50 words a draw (25 KB) and holds
 * one.  Plain C++ and vector atomics only.
 */
#include <hip/hip_runtime.h>

#include "pht_condition.h"
#include "pht_condition_args.h"
#include "pht_kernels.h"
#include "pht_layout.h"
#include "pht_unit_walk.h"

namespace pht {

static_assert(kCondMaxH == PHT_CD_MAXH, "the header's limit");
static_assert(kMaxN == 32, "the header's stack arrays");
static_assert(kCondBlock % 64 == 0 && kCondBlock >= 64 && kCondBlock <= 1024, "whole waves");

__global__ void __launch_bounds__(64) cond_forward_kernel(const CondTableArgs a) {
  const int d = blockIdx.x, lane = threadIdx.x, n = a.n;
  const double *meta = a.meta + (size_t)d * PHT_LLU_META;
  if (__double_as_longlong(meta[PHT_LLU_M_FLAG]) != 0) return; /* flagged draw: the whole wave */
  const int K = min((int)meta[PHT_LLU_M_K], a.rows - 1);
  const double rinv = 1.0 / meta[PHT_LLU_M_MU];
  const double *S = a.S + (size_t)d * n * n;
  double *F = a.F + (size_t)d * a.fstride;
  const bool col = lane < n;
  double R[kMaxN]; /* column `lane` of R */
#pragma unroll
  for (int l = 0; l < kMaxN; l++) R[l] = (col && l < n) ? pht_llu_R(S[l + lane * n], rinv, l == lane) : 0.0;
  double f = (lane == 0) ? 1.0 : 0.0;
  if (col) F[lane] = f;
  for (int k = 1; k <= K; k++) {
    double v = 0.0;
#pragma unroll
    for (int l = 0; l < kMaxN; l++) {
      if (l < n) v = fma(__shfl(f, l, 64), R[l], v);
    }
    f = v;
    if (col) F[(size_t)k * n + lane] = f;
  }
}

template <int NT, bool PW>
__global__ void __launch_bounds__(kCondBlock) cond_kernel(const CondArgs a) {
  constexpr int NV = NT ? NT : kMaxN;       /* length of v */
  constexpr int WL = NV + kCondMaxH + 2;    /* block sums a draw: the words but nunits */
  __shared__ double stab[kUnitPool];
  __shared__ double sinvk[PHT_LLU_MAXK + 1];
  __shared__ double smeta[kLoglikBatch * PHT_LLU_META];
  __shared__ unsigned long long ssum[kLoglikBatch * WL];
  const int tid = threadIdx.x, nh = a.nh, n = NT ? NT : a.n;
  const int count = (int)a.count, fstride = (int)a.fstride;
  const int nw = pht_cd_nwords(n, nh), nvec = cond_vec_doubles(n, nh);
  unit_stage<kCondBlock>(sinvk, smeta, a.meta, a.nd, a.Kmax);
  for (int k = tid; k < a.nd * WL; k += kCondBlock) ssum[k] = 0ull;
  __syncthreads();

  if constexpr (NT == 0) {
    /* runtime n: unit_walk written out with the body in place (the body in a lambda costs this build 50 to 60
     * VGPRs and 3 to 4 % of its time) */
    for (int d0 = 0; d0 < a.nd;) {
      int d1 = d0, used = 0;
      while (d1 < a.nd) {
        const double *m = smeta + d1 * PHT_LLU_META;
        const int need = (__double_as_longlong(m[PHT_LLU_M_FLAG]) != 0) ? 0 : 2 * (min((int)m[PHT_LLU_M_K], a.Kmax) + 1);
        if (used + need > kUnitPool) break;
        for (int k = tid; k < need; k += kCondBlock) stab[used + k] = a.tab[(size_t)d1 * a.stride + k];
        used += need;
        d1++;
      }
      __syncthreads();
      for (int base = (int)blockIdx.x * kCondBlock; base < count; base += (int)gridDim.x * kCondBlock) {
        const int pos = base + tid;
        const bool live = pos < count;
        const double c = live ? a.age[pos] : 1.0;
        double *st = a.state + (size_t)(live ? pos : 0) * (size_t)(n + 2 + nh);
        double *pwt = PW ? a.pw + (size_t)(live ? pos : 0) * (size_t)a.nd * (size_t)(n + 1 + nh) : nullptr;
        int off = 0;
        for (int d = d0; d < d1; d++) {
          const double *m = smeta + d * PHT_LLU_META;
          if (__double_as_longlong(m[PHT_LLU_M_FLAG]) != 0) {
            if (PW && live) {
              double *pw = pwt + (size_t)d * (size_t)(n + 1 + nh);
              for (int j = 0; j < n + 1 + nh; j++) pw[j] = NAN;
            }
            continue;
          }
          const int K = min((int)m[PHT_LLU_M_K], a.Kmax);
          const double mu = m[PHT_LLU_M_MU], abar = m[PHT_LLU_M_ABAR];
          const double *tab = stab + off;
          off += 2 * (K + 1);
#include "pht_condition_draw.inc"
        }
      }
      d0 = d1;
      __syncthreads();
    }
  } else {
    /* this lane's unit (count <= 2^22: the positions fit an int) */
    double c;
    double *st, *pwt;
    unit_walk<kCondBlock, int>(
        stab, smeta, a.tab, a.stride, a.nd, a.Kmax, count,
        [&](int pos, bool live) {
          c = live ? a.age[pos] : 1.0;
          st = a.state + (size_t)(live ? pos : 0) * (size_t)(n + 2 + nh); /* this unit's sums (good lanes only) */
          /* pointwise: this unit's [draw][phi n, MRL, D nh] */
          pwt = PW ? a.pw + (size_t)(live ? pos : 0) * (size_t)a.nd * (size_t)(n + 1 + nh) : nullptr;
        },
        [&](int d, int, bool live) {
          if (PW && live) {
            double *pw = pwt + (size_t)d * (size_t)(n + 1 + nh);
            for (int j = 0; j < n + 1 + nh; j++) pw[j] = NAN;
          }
        },
        [&](const UnitDraw &u, int, bool live) {
          const int d = u.d, K = u.K;
          const double mu = u.mu, abar = u.abar;
          const double *tab = u.tab;
#include "pht_condition_draw.inc"
        },
        [](int, bool) {});
  }
  /* the block's sums: word i of draw d (i < nw - 1: nunits is the host's) */
  for (int k = tid; k < a.nd * WL; k += kCondBlock) {
    const int d = k / WL, i = k - d * WL;
    if (i < nw - 1 && ssum[k] != 0ull) atomicAdd(a.words + (size_t)d * nw + i, ssum[k]);
  }
}

template <int NT>
static void launch_cond(const CondArgs &a, int grid, hipStream_t st) {
  if (a.pw)
    hipLaunchKernelGGL((cond_kernel<NT, true>), dim3(grid), dim3(kCondBlock), 0, st, a);
  else
    hipLaunchKernelGGL((cond_kernel<NT, false>), dim3(grid), dim3(kCondBlock), 0, st, a);
}

}  // namespace pht

extern "C" hipError_t pht_launch_cond_forward(const pht::CondTableArgs *a, hipStream_t st) {
  using namespace pht;
  if (!a || a->n < 1 || a->n > kMaxN || a->nd < 1 || a->nd > kLoglikBatch || !a->S || !a->meta || !a->F ||
      a->rows < 1 || a->rows > PHT_LLU_MAXK + 1 || a->fstride < (long)a->rows * a->n)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(cond_forward_kernel, dim3(a->nd), dim3(64), 0, st, *a);
  return hipGetLastError();
}

extern "C" hipError_t pht_launch_cond(const pht::CondArgs *a, int grid_cap, hipStream_t st) {
  using namespace pht;
  if (!a || a->n < 1 || a->n > kMaxN || a->nd < 1 || a->nd > kLoglikBatch || a->nh < 0 || a->nh > kCondMaxH ||
      a->count < 1 || a->count > PHT_CD_MAXUNITS || !a->age || !a->meta || !a->tab || !a->F || !a->vec || !a->words ||
      !a->state || grid_cap < 1 || a->Kmax < 0 || a->Kmax > PHT_LLU_MAXK || a->stride < 2 * (a->Kmax + 1) ||
      a->fstride < (long)(a->Kmax + 1) * a->n || a->fstride > (long)(PHT_LLU_MAXK + 1) * kMaxN)
    return hipErrorInvalidValue;
  const long tiles = (a->count + kCondBlock - 1) / kCondBlock;
  const int grid = (int)(tiles < (long)grid_cap ? tiles : (long)grid_cap);
  switch (a->n) {
    case 3: launch_cond<3>(*a, grid, st); break;
    case 5: launch_cond<5>(*a, grid, st); break;
    case 10: launch_cond<10>(*a, grid, st); break;
    case 15: launch_cond<15>(*a, grid, st); break;
    case 20: launch_cond<20>(*a, grid, st); break;
    default: launch_cond<0>(*a, grid, st); break;
  }
  return hipGetLastError();
}
