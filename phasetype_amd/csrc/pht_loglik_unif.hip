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
 * llunif_kernel: a unit walk (pht_unit_walk.h) over the context's sorted y,
 * one lane per observation, the WAIC state in registers over the draws of a
 * pass (reloaded per pass, the draws stay in order), wave-shuffle sums of (h,
 * f, bad, obs), one LDS add per wave and one 64-bit atomic per word and draw
 * at the end of the block.  It does not depend on n.  A pass holds one table
 * at the cap K = 2047, six to eight at K = 250 .. 310.  With the math tables
 * and invk the block stays under 64 KB, two blocks per CU.
 */
#include <hip/hip_runtime.h>

#include "pht_kernels.h"
#include "pht_layout.h"
#include "pht_loglik_unif.h"
#include "pht_loglik_unif_args.h"
#include "pht_unit_walk.h"

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
  __shared__ double stab[kUnitPool];
  __shared__ double sinvk[PHT_LLU_MAXK + 1];
  __shared__ double smeta[kLoglikBatch * PHT_LLU_META];
  __shared__ unsigned long long stot[kLoglikBatch * PHT_LL_TOT];
  const int tid = threadIdx.x;
  unit_stage<kLlunifBlock>(sinvk, smeta, a.meta, a.nd, a.Kmax);
  for (int k = tid; k < a.nd * PHT_LL_TOT; k += kLlunifBlock) stot[k] = 0ull;
  __syncthreads();

  /* this lane's observation and its WAIC state */
  double y;
  int cens;
  pht_waic_t w;
  unit_walk<kLlunifBlock, long>(
      stab, smeta, a.tab, a.stride, a.nd, a.Kmax, a.count,
      [&](long pos, bool live) {
        y = live ? a.y[pos] : 1.0;
        cens = live ? (a.cens[pos] != 0) : 0;
        w = {0.0, 0.0, 0.0, 0.0, 0.0, 0};
        if (a.acc && live) {
          w.ref = a.w_ref[pos];
          w.S1 = a.w_S1[pos];
          w.S2 = a.w_S2[pos];
          w.m = a.w_m[pos];
          w.r = a.w_r[pos];
          w.cnt = a.w_cnt[pos];
        }
      },
      [&](int d, long pos, bool live) {
        if (PW && live) a.pw[(size_t)d * (size_t)a.count + (size_t)pos] = NAN;
      },
      [&](const UnitDraw &u, long pos, bool live) {
        const int d = u.d;
        int bad, khi;
        const double l = pht_llu_eval(u.tab, sinvk, u.K, u.mu, u.abar, y, cens, &bad, &khi);
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
      },
      [&](long pos, bool live) {
        if (a.acc && live) {
          a.w_ref[pos] = w.ref;
          a.w_S1[pos] = w.S1;
          a.w_S2[pos] = w.S2;
          a.w_m[pos] = w.m;
          a.w_r[pos] = w.r;
          a.w_cnt[pos] = w.cnt;
        }
      });
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
