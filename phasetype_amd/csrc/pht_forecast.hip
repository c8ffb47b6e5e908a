/*
 * pht_forecast.hip — the fleet forecast: the conditional failure probability
 * of every censored unit of a shard at every horizon for every draw
 * (specification: include/pht_forecast.h).  The (ax, ac) tables are
 * pht_loglik_unif.hip's (pht_launch_llunif_table, with the K of the largest
 * age plus the last horizon); one kernel of its own per batch of draws.
 *
 * fcast_kernel: a unit walk (pht_unit_walk.h) over the context's censored
 * units and their sorted ages.  Per (draw, unit) one evaluation at the age,
 * then one per horizon in ascending order (a lane's successive windows
 * overlap); the loop runs j = -1 .. nh - 1 so that all of them share one copy
 * of the evaluator's loops.  Per (draw, horizon): wave-shuffle sums of (M, V,
 * bad), one LDS add per wave, one 64-bit atomic per word at the end of the
 * block (nunits = units - nbad is the host's).  A unit's qsum and cnt of every
 * horizon stay in registers over the draws of a pass, loaded and stored once
 * per pass; they are updated through a switch on the wave-uniform horizon
 * index, so every register index is a compile-time constant (no scratch).  For
 * that the kernel is built with NH = 4 and NH = 16 state slots a unit
 * (pht_fcast_slots): up to four horizons cost 12 registers of state, not 48.
 *
 * LDS: 32 KB of tables, 16 KB of 1 / k, 7 KB of math tables, 2 KB of meta
 * words and 20 KB of block sums (64 draws x 16 horizons x (8 + 8 + 4) bytes):
 * under 80 KB, two blocks a CU.  Plain C++ and vector atomics only.
 */
#include <hip/hip_runtime.h>

#include "pht_forecast.h"
#include "pht_forecast_args.h"
#include "pht_kernels.h"
#include "pht_layout.h"
#include "pht_unit_walk.h"

namespace pht {

static_assert(kFcastMaxH == PHT_FC_MAXH && kFcastMaxH == 16, "the header's limit; the switch below lists 16 cases");
static_assert(kFcastBlock % 64 == 0 && kFcastBlock >= 64 && kFcastBlock <= 1024, "whole waves");
constexpr int kFcastCells = kLoglikBatch * kFcastMaxH; /* (draw, horizon) pairs of a launch */

template <bool PW, int NH>
__global__ void __launch_bounds__(kFcastBlock) fcast_kernel(const FcastArgs a) {
  __shared__ double stab[kUnitPool];
  __shared__ double sinvk[PHT_LLU_MAXK + 1];
  __shared__ double smeta[kLoglikBatch * PHT_LLU_META];
  __shared__ unsigned long long sM[kFcastCells], sV[kFcastCells];
  __shared__ unsigned sB[kFcastCells];
  __shared__ double sh[kFcastMaxH];
  const int tid = threadIdx.x, nh = a.nh;
  unit_stage<kFcastBlock>(sinvk, smeta, a.meta, a.nd, a.Kmax);
  if (tid < nh) sh[tid] = a.h[tid];
  for (int k = tid; k < a.nd * nh; k += kFcastBlock) {
    sM[k] = 0ull;
    sV[k] = 0ull;
    sB[k] = 0u;
  }
  __syncthreads();

  /* this lane's unit: its age and its state, NH slots a unit on the device (the slots past nh stay 0) */
  double c;
  double qs[NH];
  int cn[NH];
  unit_walk<kFcastBlock, long>(
      stab, smeta, a.tab, a.stride, a.nd, a.Kmax, a.count,
      [&](long pos, bool live) {
        c = live ? a.age[pos] : 1.0;
#pragma unroll
        for (int t = 0; t < NH; t++) {
          qs[t] = live ? a.qsum[(size_t)pos * NH + t] : 0.0;
          cn[t] = live ? a.cnt[(size_t)pos * NH + t] : 0;
        }
      },
      [&](int d, long pos, bool live) {
        if (PW && live)
          for (int j = 0; j < nh; j++) a.q[((size_t)d * (size_t)a.count + (size_t)pos) * nh + j] = NAN;
      },
      [&](const UnitDraw &u, long pos, bool live) {
        const int d = u.d, K = u.K;
        const double mu = u.mu, abar = u.abar;
        const double *tab = u.tab;
        int bad0 = 0;
        double l0 = 0.0;
        for (int j = -1; j < nh; j++) { /* j = -1: the age itself (one copy of the evaluator's loops) */
          int badj, khi, bad;
          const double lj = pht_llu_eval(tab, sinvk, K, mu, abar, pht_fc_y(c, sh, j), 1, &badj, &khi);
          if (j < 0) {
            l0 = lj;
            bad0 = badj;
            continue;
          }
          const double q = pht_fc_pair(l0, bad0, lj, badj, &bad);
          long long mw = 0, vw = 0;
          int bw = 0;
          const bool good = live && !bad;
          if (good) pht_fc_fixed(q, &mw, &vw);
          bw = (live && bad) ? 1 : 0;
          /* qs[j] += q, cn[j] += 1 in the good lanes, through compile-time
           * indices (j is the same in every lane: a scalar branch; adding +0
           * elsewhere leaves the bits, qs is never -0) */
          const double qadd = good ? q : 0.0;
          const int cadd = good ? 1 : 0;
          switch (j) {
#define PHT_FC_CASE(t)        \
  case t:                     \
    if constexpr (t < NH) {   \
      qs[t] = qs[t] + qadd;   \
      cn[t] = cn[t] + cadd;   \
    }                         \
    break;
            PHT_FC_CASE(0) PHT_FC_CASE(1) PHT_FC_CASE(2) PHT_FC_CASE(3) PHT_FC_CASE(4) PHT_FC_CASE(5) PHT_FC_CASE(6)
            PHT_FC_CASE(7) PHT_FC_CASE(8) PHT_FC_CASE(9) PHT_FC_CASE(10) PHT_FC_CASE(11) PHT_FC_CASE(12)
            PHT_FC_CASE(13) PHT_FC_CASE(14) PHT_FC_CASE(15)
#undef PHT_FC_CASE
            default:
              break;
          }
          if (PW && live) a.q[((size_t)d * (size_t)a.count + (size_t)pos) * nh + j] = q;
          mw = wave_sum(mw);
          vw = wave_sum(vw);
          bw = wave_sum(bw);
          if ((tid & 63) == 0) {
            const int cell = d * nh + j;
            atomicAdd(sM + cell, (unsigned long long)mw);
            atomicAdd(sV + cell, (unsigned long long)vw);
            atomicAdd(sB + cell, (unsigned)bw);
          }
        }
      },
      [&](long pos, bool live) {
        if (live) {
#pragma unroll
          for (int t = 0; t < NH; t++) {
            a.qsum[(size_t)pos * NH + t] = qs[t];
            a.cnt[(size_t)pos * NH + t] = cn[t];
          }
        }
      });
  for (int k = tid; k < a.nd * nh; k += kFcastBlock) {
    unsigned long long *w = a.words + (size_t)k * PHT_FC_WORDS;
    if (sM[k] != 0ull) atomicAdd(w + PHT_FC_W_M, sM[k]);
    if (sV[k] != 0ull) atomicAdd(w + PHT_FC_W_V, sV[k]);
    if (sB[k] != 0u) atomicAdd(w + PHT_FC_W_NBAD, (unsigned long long)sB[k]);
  }
}

}  // namespace pht

extern "C" int pht_fcast_slots(int nh) { return nh <= pht::kFcastFewH ? pht::kFcastFewH : pht::kFcastMaxH; }

extern "C" hipError_t pht_launch_fcast(const pht::FcastArgs *a, int grid_cap, hipStream_t st) {
  using namespace pht;
  if (!a || a->nd < 1 || a->nd > kLoglikBatch || a->nh < 1 || a->nh > kFcastMaxH || a->count < 1 ||
      a->count > PHT_FC_MAXUNITS || !a->age || !a->h || !a->meta || !a->tab || !a->words || !a->qsum || !a->cnt ||
      grid_cap < 1 || a->Kmax < 0 || a->Kmax > PHT_LLU_MAXK || a->stride < 2 * (a->Kmax + 1))
    return hipErrorInvalidValue;
  const long tiles = (a->count + kFcastBlock - 1) / kFcastBlock;
  const int grid = (int)(tiles < (long)grid_cap ? tiles : (long)grid_cap);
  const bool few = pht_fcast_slots(a->nh) == kFcastFewH;
  if (a->q && few)
    hipLaunchKernelGGL((fcast_kernel<true, kFcastFewH>), dim3(grid), dim3(kFcastBlock), 0, st, *a);
  else if (a->q)
    hipLaunchKernelGGL((fcast_kernel<true, kFcastMaxH>), dim3(grid), dim3(kFcastBlock), 0, st, *a);
  else if (few)
    hipLaunchKernelGGL((fcast_kernel<false, kFcastFewH>), dim3(grid), dim3(kFcastBlock), 0, st, *a);
  else
    hipLaunchKernelGGL((fcast_kernel<false, kFcastMaxH>), dim3(grid), dim3(kFcastBlock), 0, st, *a);
  return hipGetLastError();
}
