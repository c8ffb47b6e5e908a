/*
 * pht_loglik_unif.hip — the log-likelihood of posterior draws by
 * uniformisation over a shard's resident observations (specification:
 * include/pht_loglik_unif.h).  Two kernels per batch of draws.
 *
 * llunif_table_kernel: one wavefront per draw.  Lane i keeps row i of R in
 * registers with B[i] and C[i]; B_{k-1}[j] reaches every lane by a wave
 * shuffle in increasing j (no LDS round trip, no barrier); lane 0 stores
 * (ax_k, ac_k).  K dependent steps.
 *
 * llunif_kernel: pht_loglik.hip's structure — one lane per observation over
 * the context's sorted y, tiles over a capped grid, the WAIC state in
 * registers over the draws of a pass, wave-shuffle sums of (h, f, bad, obs),
 * one LDS add per wave and one 64-bit atomic per word and draw at the end of
 * the block; lanes past the last observation are masked, never returned
 * early.  It does not depend on n.  The hot loop reads invk[k] and the
 * interleaved (ax_k, ac_k) from LDS: the launch's draws are taken in passes of
 * as many whole tables as fit kLlunifPool doubles (one table at the cap
 * K = 2047, six to eight at K = 250 .. 310); the WAIC state is reloaded per
 * pass, the draws stay in order.  With the math tables and invk the block
 * stays under 64 KB, two blocks per CU.  y is sorted, so neighbouring lanes
 * walk neighbouring k.
 */
#include <hip/hip_runtime.h>

#include "pht_kernels.h"
#include "pht_layout.h"
#include "pht_loglik_unif.h"
#include "pht_loglik_unif_args.h"

namespace pht {

static_assert(PHT_LLU_MAXK == kUnifMaxK, "the evaluator's table cap is the sampler's");

/* lanes of a block (= observations of a tile).  The LDS of a block allows two
 * blocks a CU whatever their size, so the block size sets the waves in
 * flight: 512 lanes are 4 waves a SIMD (256: 2, PHT_LLUNIF_BLOCK=256 for the
 * A/B in DESIGN.md 5d) */
#ifndef PHT_LLUNIF_BLOCK
#define PHT_LLUNIF_BLOCK 512
#endif
constexpr int kLlunifBlock = PHT_LLUNIF_BLOCK;
static_assert(kLlunifBlock % 64 == 0 && kLlunifBlock >= 64 && kLlunifBlock <= 1024, "whole waves");
constexpr int kLlunifPool = 2 * (PHT_LLU_MAXK + 1); /* doubles of table per pass */

__device__ __forceinline__ long long llu_wave_sum(long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ void __launch_bounds__(64) llunif_table_kernel(const LlunifTableArgs a) {
  const int d = blockIdx.x, lane = threadIdx.x, n = a.n;
  const double *meta = a.meta + (size_t)d * PHT_LLU_META;
  if (__double_as_longlong(meta[PHT_LLU_M_FLAG]) != 0) return; /* flagged draw: the whole wave */
  const int K = min((int)meta[PHT_LLU_M_K], a.stride / 2 - 1); /* (the host sizes stride for the largest K) */
  const double rinv = 1.0 / meta[PHT_LLU_M_MU];
  const double *S = a.S + (size_t)d * n * n, *s = a.s + (size_t)d * n;
  double *tab = a.tab + (size_t)d * a.stride;
  const bool row = lane < n;
  double R[kMaxN];
#pragma unroll
  for (int j = 0; j < kMaxN; j++) R[j] = (row && j < n) ? pht_llu_R(S[lane + j * n], rinv, lane == j) : 0.0;
  double B = row ? s[lane] : 0.0, Cv = row ? 1.0 : 0.0;
  if (lane == 0) {
    tab[0] = B;
    tab[1] = Cv;
  }
  for (int k = 1; k <= K; k++) {
    double b = 0.0, c = 0.0;
#pragma unroll
    for (int j = 0; j < kMaxN; j++) {
      if (j < n) {
        b = fma(R[j], __shfl(B, j, 64), b);
        c = fma(R[j], __shfl(Cv, j, 64), c);
      }
    }
    B = b;
    Cv = c;
    if (lane == 0) {
      tab[2 * k] = B;
      tab[2 * k + 1] = Cv;
    }
  }
}

template <bool PW>
__global__ void __launch_bounds__(kLlunifBlock) llunif_kernel(const LlunifArgs a) {
  __shared__ double stab[kLlunifPool];
  __shared__ double sinvk[PHT_LLU_MAXK + 1];
  __shared__ double smeta[kLoglikBatch * PHT_LLU_META];
  __shared__ unsigned long long stot[kLoglikBatch * PHT_LL_TOT];
  const int tid = threadIdx.x;
  pht_stage_math_tables();
  for (int k = tid; k <= a.Kmax; k += kLlunifBlock) sinvk[k] = k ? 1.0 / (double)k : 0.0;
  for (int k = tid; k < a.nd * PHT_LLU_META; k += kLlunifBlock) smeta[k] = a.meta[k];
  for (int k = tid; k < a.nd * PHT_LL_TOT; k += kLlunifBlock) stot[k] = 0ull;
  __syncthreads();

  for (int d0 = 0; d0 < a.nd;) {
    /* this pass: draws [d0, d1), as many whole tables as fit the pool (the
     * same count in every lane; a flagged draw takes no room) */
    int d1 = d0, used = 0;
    while (d1 < a.nd) {
      const double *m = smeta + d1 * PHT_LLU_META;
      const int need = (__double_as_longlong(m[PHT_LLU_M_FLAG]) != 0) ? 0 : 2 * (min((int)m[PHT_LLU_M_K], a.Kmax) + 1);
      if (used + need > kLlunifPool) break;
      for (int k = tid; k < need; k += kLlunifBlock) stab[used + k] = a.tab[(size_t)d1 * a.stride + k];
      used += need;
      d1++;
    }
    __syncthreads();

    for (long base = (long)blockIdx.x * kLlunifBlock; base < a.count; base += (long)gridDim.x * kLlunifBlock) {
      const long pos = base + tid;
      const bool live = pos < a.count;
      const double y = live ? a.y[pos] : 1.0;
      const int cens = live ? (a.cens[pos] != 0) : 0;
      pht_waic_t w = {0.0, 0.0, 0.0, 0.0, 0.0, 0};
      if (a.acc && live) {
        w.ref = a.w_ref[pos];
        w.S1 = a.w_S1[pos];
        w.S2 = a.w_S2[pos];
        w.m = a.w_m[pos];
        w.r = a.w_r[pos];
        w.cnt = a.w_cnt[pos];
      }
      int off = 0;
      for (int d = d0; d < d1; d++) {
        const double *m = smeta + d * PHT_LLU_META;
        if (__double_as_longlong(m[PHT_LLU_M_FLAG]) != 0) { /* unusable draw: the same for every lane */
          if (PW && live) a.pw[(size_t)d * (size_t)a.count + (size_t)pos] = NAN;
          continue;
        }
        const int K = min((int)m[PHT_LLU_M_K], a.Kmax);
        int bad, khi;
        const double l = pht_llu_eval(stab + off, sinvk, K, m[PHT_LLU_M_MU], m[PHT_LLU_M_ABAR], y, cens, &bad, &khi);
        off += 2 * (K + 1);
        long long h = 0, f = 0, bo = 0; /* bo: bad << 32 | obs (a wave adds at most 64 of each) */
        if (live) {
          if (bad) {
            bo = 1ll << 32;
          } else {
            pht_ll_fixed(l, &h, &f);
            bo = 1;
            if (a.acc) pht_waic_update(&w, l);
          }
          if (PW) a.pw[(size_t)d * (size_t)a.count + (size_t)pos] = l;
        }
        h = llu_wave_sum(h);
        f = llu_wave_sum(f);
        bo = llu_wave_sum(bo);
        if ((tid & 63) == 0) {
          unsigned long long *t = stot + d * PHT_LL_TOT;
          atomicAdd(t + 0, (unsigned long long)h);
          atomicAdd(t + 1, (unsigned long long)f);
          atomicAdd(t + 2, (unsigned long long)(bo >> 32));
          atomicAdd(t + 3, (unsigned long long)(bo & 0xffffffffll));
        }
      }
      if (a.acc && live) {
        a.w_ref[pos] = w.ref;
        a.w_S1[pos] = w.S1;
        a.w_S2[pos] = w.S2;
        a.w_m[pos] = w.m;
        a.w_r[pos] = w.r;
        a.w_cnt[pos] = w.cnt;
      }
    }
    d0 = d1;
    __syncthreads(); /* every lane is done with this pass's tables */
  }
  for (int k = tid; k < a.nd * PHT_LL_TOT; k += kLlunifBlock)
    if (stot[k] != 0ull) atomicAdd(a.totals + k, stot[k]);
}

}  // namespace pht

extern "C" hipError_t pht_launch_llunif_table(const pht::LlunifTableArgs *a, hipStream_t st) {
  using namespace pht;
  if (!a || a->n < 1 || a->n > kMaxN || a->nd < 1 || a->nd > kLoglikBatch || !a->S || !a->s || !a->meta || !a->tab ||
      a->stride < 2 || a->stride > 2 * (PHT_LLU_MAXK + 1))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(llunif_table_kernel, dim3(a->nd), dim3(64), 0, st, *a);
  return hipGetLastError();
}

extern "C" hipError_t pht_launch_llunif(const pht::LlunifArgs *a, int grid_cap, hipStream_t st) {
  using namespace pht;
  if (!a || a->nd < 1 || a->nd > kLoglikBatch || a->count < 1 || !a->y || !a->cens || !a->meta || !a->tab ||
      !a->totals || grid_cap < 1 || a->Kmax < 0 || a->Kmax > PHT_LLU_MAXK || a->stride < 2 * (a->Kmax + 1))
    return hipErrorInvalidValue;
  if (a->acc && !(a->w_ref && a->w_S1 && a->w_S2 && a->w_m && a->w_r && a->w_cnt)) return hipErrorInvalidValue;
  const long tiles = (a->count + kLlunifBlock - 1) / kLlunifBlock;
  const int grid = (int)(tiles < (long)grid_cap ? tiles : (long)grid_cap);
  if (a->pw)
    hipLaunchKernelGGL((llunif_kernel<true>), dim3(grid), dim3(kLlunifBlock), 0, st, *a);
  else
    hipLaunchKernelGGL((llunif_kernel<false>), dim3(grid), dim3(kLlunifBlock), 0, st, *a);
  return hipGetLastError();
}
