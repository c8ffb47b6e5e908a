/*
 * pht_loglik.hip — observed-data log-likelihood of posterior draws over a
 * shard's resident observations (specification: include/pht_loglik.h).
 *
 * One lane per observation, tiles of 256 over a capped grid.  The launch's
 * draw blocks (up to kLoglikBatch) are staged once per workgroup in LDS; a
 * block's words are the same for every lane, so its reads are broadcasts.
 * Per draw a lane evaluates l (the n exponentials first, then the two
 * dependent fma chains: the sum and the cancellation guard's sum of absolute
 * terms), updates its private WAIC state and contributes (h, f, bad, obs)
 * to the draw's totals: wave shuffles, then one LDS add per wave, and at the
 * end of the block one 64-bit integer atomic per word and draw.  Integer sums:
 * the totals do not depend on the grid, the tiling or the batch.
 *
 * Lanes past the last observation stay in the loop with a dummy y and are
 * masked out of every sum and store (no return before a barrier or shuffle).
 */
#include <hip/hip_runtime.h>

#include "pht_layout.h"
#include "pht_loglik.h"
#include "pht_loglik_args.h"
#include "pht_wave.h"

namespace pht {

constexpr int kLoglikBlock = 256;

template <int NT, bool PW>
__global__ void __launch_bounds__(kLoglikBlock) loglik_kernel(const LoglikArgs a) {
  constexpr int kWords = 2 + 3 * (NT ? NT : kMaxN);
  __shared__ double sblk[kLoglikBatch * kWords];
  __shared__ unsigned long long stot[kLoglikBatch * PHT_LL_TOT];
  const int n = NT ? NT : a.n;
  const int words = 2 + 3 * n;
  const int tid = threadIdx.x;
  pht_stage_math_tables();
  for (int k = tid; k < a.nd * words; k += kLoglikBlock) sblk[k] = a.blocks[k];
  for (int k = tid; k < a.nd * PHT_LL_TOT; k += kLoglikBlock) stot[k] = 0ull;
  __syncthreads();

  for (long base = (long)blockIdx.x * kLoglikBlock; base < a.count; base += (long)gridDim.x * kLoglikBlock) {
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
    for (int d = 0; d < a.nd; d++) {
      const double *blk = sblk + d * words;
      if (__double_as_longlong(blk[PHT_LL_FLAG]) != 0) { /* unusable draw: the same for every lane */
        if (PW && live) a.pw[(size_t)d * (size_t)a.count + (size_t)pos] = NAN;
        continue;
      }
      const double *dl = blk + PHT_LL_DL;
      const double *c = blk + PHT_LL_DL + (cens ? 2 * n : n);
      double acc = 0.0, accabs = 0.0; /* accabs: the cancellation guard's sum of |c_i| e_i */
      if constexpr (NT > 0) {
        double e[NT > 0 ? NT : 1];
#pragma unroll
        for (int i = 0; i < NT; i++) e[i] = pht_ll_expterm(dl[i], y);
#pragma unroll
        for (int i = 0; i < NT; i++) {
          acc = fma(c[i], e[i], acc);
          accabs = fma(fabs(c[i]), e[i], accabs);
        }
      } else {
        for (int i = 0; i < n; i++) {
          const double e = pht_ll_expterm(dl[i], y);
          acc = fma(c[i], e, acc);
          accabs = fma(fabs(c[i]), e, accabs);
        }
      }
      int bad;
      const double l = pht_ll_finish(blk[PHT_LL_LMAX], y, acc, accabs, &bad);
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
      h = wave_sum(h);
      f = wave_sum(f);
      bo = wave_sum(bo);
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
  __syncthreads();
  for (int k = tid; k < a.nd * PHT_LL_TOT; k += kLoglikBlock)
    if (stot[k] != 0ull) atomicAdd(a.totals + k, stot[k]);
}

template <int NT>
static hipError_t launch_nt(const LoglikArgs &a, int grid, hipStream_t st) {
  if (a.pw)
    hipLaunchKernelGGL((loglik_kernel<NT, true>), dim3(grid), dim3(kLoglikBlock), 0, st, a);
  else
    hipLaunchKernelGGL((loglik_kernel<NT, false>), dim3(grid), dim3(kLoglikBlock), 0, st, a);
  return hipGetLastError();
}

}  // namespace pht

extern "C" hipError_t pht_launch_loglik(const pht::LoglikArgs *a, int grid_cap, hipStream_t st) {
  using namespace pht;
  if (!a || a->n < 1 || a->n > kMaxN || a->nd < 1 || a->nd > kLoglikBatch || a->count < 1 || !a->y || !a->cens ||
      !a->blocks || !a->totals || grid_cap < 1)
    return hipErrorInvalidValue;
  if (a->acc && !(a->w_ref && a->w_S1 && a->w_S2 && a->w_m && a->w_r && a->w_cnt)) return hipErrorInvalidValue;
  const long tiles = (a->count + kLoglikBlock - 1) / kLoglikBlock;
  const int grid = (int)(tiles < (long)grid_cap ? tiles : (long)grid_cap);
  switch (a->n) {
    case 3: return launch_nt<3>(*a, grid, st);
    case 5: return launch_nt<5>(*a, grid, st);
    case 10: return launch_nt<10>(*a, grid, st);
    case 15: return launch_nt<15>(*a, grid, st);
    case 20: return launch_nt<20>(*a, grid, st);
    default: return launch_nt<0>(*a, grid, st);
  }
}
