/*
 * pht_spares.hip — the fleet spares: for every draw, every censored unit of a
 * shard and every horizon the mean and the variance of the unit's failures
 * with replacement (specification: include/pht_spares.h).  The (ax, ac) tables
 * are pht_loglik_unif.hip's (pht_launch_llunif_table, with the K of the largest
 * age) and the forward tables pht_condition.hip's (pht_launch_cond_forward);
 * two kernels of its own per batch of draws.  Unlike the condition, the draw's
 * vectors are built HERE, not on the host: n^2 (Kr + 1) operations a draw,
 * three times over (u, a, b), one wavefront a draw.
 *
 * spares_vectors_kernel: one wavefront per draw.  First the weights, serial in
 * k: lane j < nh runs pht_sp_weights for horizon j into the draw's scratch in
 * global memory, W[k][j][T, p] (neighbouring lanes write neighbouring
 * addresses), and the wave meets at a barrier.  Then lane i keeps row i of P*
 * in registers with u[i], a[i], b[i] and the 2 nh accumulators r_j[i], q_j[i];
 * u, a and b reach every lane by wave shuffles in increasing j; the 2 nh
 * weights of step k are read by the first 2 nh lanes in one load (the next
 * step's ahead of the matrix-vector products) and handed round by shuffles.
 * Kr dependent steps.  Lane i stores r[.][i] and q[.][i]; the scales' maxima
 * are taken in the header's order (i increasing), the same in every lane.
 *
 * spares_kernel: pht_condition.hip's cond_kernel with other words — a unit
 * walk (pht_unit_walk.h) over the context's censored units, the first pass
 * over a unit's window from LDS, the rows F[k][.] of the second pass through
 * the caches, v[n] in registers: built for n = 3, 5, 10, 15, 20 and once for a
 * runtime n up to 32.  Per draw and word: a wave-shuffle sum, one LDS add per
 * wave, one 64-bit atomic per word at the end of the block (nunits = units -
 * nbad is the host's).  A unit's sums and its count live in global memory,
 * [unit][word], read and written by the owning lane once per draw in which the
 * unit is good: in draw order.
 *
 * LDS: 32 KB of tables, 16 KB of 1 / k, 7 KB of math tables, 2 KB of meta
 * words and 16.5 KB of block sums (64 draws x 33 words, whatever n): under
 * 80 KB, two blocks a CU.  Plain C++ and vector atomics only.
 */
#include <hip/hip_runtime.h>

#include "pht_kernels.h"
#include "pht_layout.h"
#include "pht_spares.h"
#include "pht_spares_args.h"
#include "pht_unit_walk.h"

namespace pht {

static_assert(kSparesMaxH == PHT_CD_MAXH, "the header's limit");
static_assert(kMaxN == 32, "the header's stack arrays");
static_assert(2 * kSparesMaxH <= 64, "a step's weights fit one wave");
static_assert(kSparesBlock % 64 == 0 && kSparesBlock >= 64 && kSparesBlock <= 1024, "whole waves");
constexpr int kSparesWL = 2 * kSparesMaxH + 1;      /* block sums a draw: Delta, V at fixed places, nbad */

__global__ void __launch_bounds__(64) spares_vectors_kernel(const SparesVecArgs a) {
  const int d = blockIdx.x, lane = threadIdx.x, n = a.n, nh = a.nh;
  const double *meta = a.meta + (size_t)d * PHT_LLU_META;
  if (__double_as_longlong(meta[PHT_LLU_M_FLAG]) != 0) return; /* flagged draw: the whole wave */
  const double mu = meta[PHT_LLU_M_MU], rinv = 1.0 / mu;
  const int Kr = max(0, min(a.kr[d], a.rows - 1));
  double *W = a.W + (size_t)d * a.wstride;
  if (lane < nh) pht_sp_weights(mu, a.h[lane], Kr, nh, lane, W);
  __syncthreads(); /* the weights are written (one wave a block) */

  const double *S = a.S + (size_t)d * n * n;
  const bool row = lane < n;
  double P[kMaxN]; /* row `lane` of P* */
#pragma unroll
  for (int l = 0; l < kMaxN; l++) P[l] = (row && l < n) ? pht_llu_R(S[lane + l * n], rinv, l == lane) : 0.0;
  const double sv = row ? a.s[(size_t)d * n + lane] : 0.0;
  const double c = sv * rinv, c2 = 2.0 * c;
  P[0] = P[0] + c;
  double u = sv, av = 0.0, bv = 0.0;
  double r[kSparesMaxH], q[kSparesMaxH];
#pragma unroll
  for (int j = 0; j < kSparesMaxH; j++) r[j] = q[j] = 0.0;
  const int nw2 = 2 * nh;
  const bool wl_lane = lane < nw2;
  double wl = wl_lane ? W[lane] : 0.0; /* (T_k, p_k) of horizon lane / 2, k = 0 */
  for (int k = 0; k <= Kr; k++) {
    const double wn = (wl_lane && k < Kr) ? W[(size_t)(k + 1) * nw2 + lane] : 0.0;
    if (k) {
      const double b0 = __shfl(bv, 0, 64);
      double vu = 0.0, va = c2 * b0, vb = c;
#pragma unroll
      for (int l = 0; l < kMaxN; l++) {
        if (l < n) {
          vu = fma(P[l], __shfl(u, l, 64), vu);
          va = fma(P[l], __shfl(av, l, 64), va);
          vb = fma(P[l], __shfl(bv, l, 64), vb);
        }
      }
      u = vu;
      av = va;
      bv = vb;
    }
#pragma unroll
    for (int j = 0; j < kSparesMaxH; j++) {
      if (j < nh) {
        r[j] = fma(__shfl(wl, 2 * j, 64), u, r[j]);
        q[j] = fma(__shfl(wl, 2 * j + 1, 64), av, q[j]);
      }
    }
    wl = wn;
  }
  double *vec = a.vec + (size_t)d * spares_vec_doubles(n, nh);
#pragma unroll
  for (int j = 0; j < kSparesMaxH; j++) {
    if (j < nh) {
      r[j] = rinv * r[j];
      if (row) {
        vec[j * n + lane] = r[j];
        vec[(nh + j) * n + lane] = q[j];
      }
      double mr = 0.0, mv = 0.0;
#pragma unroll
      for (int i = 0; i < kMaxN; i++) {
        if (i < n) {
          const double x = __shfl(r[j], i, 64), y = __shfl(q[j], i, 64) + x;
          mr = (x > mr) ? x : mr;
          mv = (y > mv) ? y : mv;
        }
      }
      if (lane == 0) {
        vec[2 * nh * n + j] = pht_es_yscale(mr);
        vec[2 * nh * n + nh + j] = pht_es_yscale(mv);
      }
    }
  }
}

template <int NT, bool PW>
__global__ void __launch_bounds__(kSparesBlock) spares_kernel(const SparesArgs a) {
  constexpr int NV = NT ? NT : kMaxN; /* length of v */
  constexpr int WL = kSparesWL;
  __shared__ double stab[kUnitPool];
  __shared__ double sinvk[PHT_LLU_MAXK + 1];
  __shared__ double smeta[kLoglikBatch * PHT_LLU_META];
  __shared__ unsigned long long ssum[kLoglikBatch * WL];
  const int tid = threadIdx.x, nh = a.nh, n = NT ? NT : a.n;
  const int count = (int)a.count, fstride = (int)a.fstride;
  const int nw = pht_sp_nwords(nh), nvec = spares_vec_doubles(n, nh), ns = 3 * nh + 1;
  unit_stage<kSparesBlock>(sinvk, smeta, a.meta, a.nd, a.Kmax);
  for (int k = tid; k < a.nd * WL; k += kSparesBlock) ssum[k] = 0ull;
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
        for (int k = tid; k < need; k += kSparesBlock) stab[used + k] = a.tab[(size_t)d1 * a.stride + k];
        used += need;
        d1++;
      }
      __syncthreads();
      for (int base = (int)blockIdx.x * kSparesBlock; base < count; base += (int)gridDim.x * kSparesBlock) {
        const int pos = base + tid;
        const bool live = pos < count;
        const double c = live ? a.age[pos] : 1.0;
        double *st = a.state + (size_t)(live ? pos : 0) * (size_t)ns;
        double *pwt = PW ? a.pw + (size_t)(live ? pos : 0) * (size_t)a.nd * (size_t)(2 * nh) : nullptr;
        int off = 0;
        for (int d = d0; d < d1; d++) {
          const double *m = smeta + d * PHT_LLU_META;
          if (__double_as_longlong(m[PHT_LLU_M_FLAG]) != 0) {
            if (PW && live) {
              double *pw = pwt + (size_t)d * (size_t)(2 * nh);
              for (int j = 0; j < 2 * nh; j++) pw[j] = NAN;
            }
            continue;
          }
          const int K = min((int)m[PHT_LLU_M_K], a.Kmax);
          const double mu = m[PHT_LLU_M_MU], abar = m[PHT_LLU_M_ABAR];
          const double *tab = stab + off;
          off += 2 * (K + 1);
#include "pht_spares_draw.inc"
        }
      }
      d0 = d1;
      __syncthreads();
    }
  } else {
    /* this lane's unit (count <= 2^22: the positions fit an int) */
    double c;
    double *st, *pwt;
    unit_walk<kSparesBlock, int>(
        stab, smeta, a.tab, a.stride, a.nd, a.Kmax, count,
        [&](int pos, bool live) {
          c = live ? a.age[pos] : 1.0;
          st = a.state + (size_t)(live ? pos : 0) * (size_t)ns; /* this unit's sums (good lanes only) */
          /* pointwise: this unit's [draw][D nh, var nh] */
          pwt = PW ? a.pw + (size_t)(live ? pos : 0) * (size_t)a.nd * (size_t)(2 * nh) : nullptr;
        },
        [&](int d, int, bool live) {
          if (PW && live) {
            double *pw = pwt + (size_t)d * (size_t)(2 * nh);
            for (int j = 0; j < 2 * nh; j++) pw[j] = NAN;
          }
        },
        [&](const UnitDraw &u, int, bool live) {
          const int d = u.d, K = u.K;
          const double mu = u.mu, abar = u.abar;
          const double *tab = u.tab;
#include "pht_spares_draw.inc"
        },
        [](int, bool) {});
  }
  /* the block's sums: place i of draw d -> word Delta_i, V_{i - 16} or nbad (nunits is the host's) */
  for (int k = tid; k < a.nd * WL; k += kSparesBlock) {
    const int d = k / WL, i = k - d * WL;
    int w = -1;
    if (i < nh) w = pht_sp_w_D(i);
    else if (i >= kSparesMaxH && i < kSparesMaxH + nh) w = pht_sp_w_V(nh, i - kSparesMaxH);
    else if (i == 2 * kSparesMaxH) w = pht_sp_w_nbad(nh);
    if (w >= 0 && ssum[k] != 0ull) atomicAdd(a.words + (size_t)d * nw + w, ssum[k]);
  }
}

template <int NT>
static void launch_spares(const SparesArgs &a, int grid, hipStream_t st) {
  if (a.pw)
    hipLaunchKernelGGL((spares_kernel<NT, true>), dim3(grid), dim3(kSparesBlock), 0, st, a);
  else
    hipLaunchKernelGGL((spares_kernel<NT, false>), dim3(grid), dim3(kSparesBlock), 0, st, a);
}

}  // namespace pht

extern "C" hipError_t pht_launch_spares_vectors(const pht::SparesVecArgs *a, hipStream_t st) {
  using namespace pht;
  if (!a || a->n < 1 || a->n > kMaxN || a->nd < 1 || a->nd > kLoglikBatch || a->nh < 1 || a->nh > kSparesMaxH ||
      !a->S || !a->s || !a->meta || !a->h || !a->kr || !a->W || !a->vec || a->rows < 1 ||
      a->rows > PHT_LLU_MAXK + 1 || a->wstride < (long)PHT_SP_WDOUBLES(a->nh, a->rows))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(spares_vectors_kernel, dim3(a->nd), dim3(64), 0, st, *a);
  return hipGetLastError();
}

extern "C" hipError_t pht_launch_spares(const pht::SparesArgs *a, int grid_cap, hipStream_t st) {
  using namespace pht;
  if (!a || a->n < 1 || a->n > kMaxN || a->nd < 1 || a->nd > kLoglikBatch || a->nh < 1 || a->nh > kSparesMaxH ||
      a->count < 1 || a->count > PHT_CD_MAXUNITS || !a->age || !a->meta || !a->tab || !a->F || !a->vec || !a->words ||
      !a->state || grid_cap < 1 || a->Kmax < 0 || a->Kmax > PHT_LLU_MAXK || a->stride < 2 * (a->Kmax + 1) ||
      a->fstride < (long)(a->Kmax + 1) * a->n || a->fstride > (long)(PHT_LLU_MAXK + 1) * kMaxN)
    return hipErrorInvalidValue;
  const long tiles = (a->count + kSparesBlock - 1) / kSparesBlock;
  const int grid = (int)(tiles < (long)grid_cap ? tiles : (long)grid_cap);
  switch (a->n) {
    case 3: launch_spares<3>(*a, grid, st); break;
    case 5: launch_spares<5>(*a, grid, st); break;
    case 10: launch_spares<10>(*a, grid, st); break;
    case 15: launch_spares<15>(*a, grid, st); break;
    case 20: launch_spares<20>(*a, grid, st); break;
    default: launch_spares<0>(*a, grid, st); break;
  }
  return hipGetLastError();
}
