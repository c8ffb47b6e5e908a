/*
 * pht_predict.hip — posterior-predictive replicates: the chain of each draw
 * run forward to absorption and the exact integer reductions of the
 * absorption times (specification: include/pht_predict.h).
 *
 * ppred_kernel: blockIdx.y is the draw, blockIdx.x one of the blocks that share
 * its replicates.  The block stages the draw's table (scale[n] and cum[n][n],
 * the rows padded to an odd leading dimension: lanes in different states read
 * different banks, lanes in one state one broadcast address), the edges and a
 * zeroed histogram in LDS.  Its lanes are persistent over a static stripe of
 * the replicates (replicate = lane index + k * lanes of the draw): a wave runs
 * rounds of kPpredJumps jumps; at the end of a round, a wave-uniform point,
 * the lanes whose path ended record it (fixed-point words in registers, the
 * bin by binary search in LDS, one LDS histogram add) and start their next
 * replicate, so no lane waits for the longest path of its wave, only for the
 * end of its round.  Every lane starts its streams at a round's top and draws
 * two words per jump, so the wave's lanes need their next Philox block at the
 * same jump (pht_stream_topup at the top of every second jump).  Every
 * replicate owns its stream: which lane takes it changes nothing.
 * Totals: wave shuffles, one LDS add per wave, one 64-bit atomic per word and
 * draw at the end of the block (pht_loglik.hip's structure); lanes past the
 * last replicate are masked, never returned early.  Runtime n <= 32.
 */
#include <hip/hip_runtime.h>

#include "pht_device.h"
#include "pht_predict.h"
#include "pht_predict_args.h"
#include "pht_wave.h"

namespace pht {

static_assert(PHT_PRED_MAXJUMPS == kMaxJumps, "the replicates' jump cap is the samplers'");
static_assert(PHT_PRED_MAXN == kMaxN, "runtime n up to the samplers' ceiling");
static_assert(kPpredBlock % 64 == 0, "whole waves");

/* jumps of a round (between two wave-uniform record-and-restart points): a
 * longer round pays the record-and-restart code less often and leaves an
 * ended lane idle longer ((kPpredJumps - 1) / 2 jumps a path on average).
 * 4 against 2: -4.5 / -6.6 / -6.0 % per call at BD-exit(3 / 10 / 20), 3.3 /
 * 7.4 / 8.8 jumps a path; 1: +33 % at n = 10 */
#ifndef PHT_PPRED_JUMPS
#define PHT_PPRED_JUMPS 4
#endif
constexpr int kPpredJumps = PHT_PPRED_JUMPS;
constexpr int kPpredLd = PHT_PRED_MAXN + 1; /* the largest padded leading dimension */

__device__ __forceinline__ unsigned long long ppred_wave_min(unsigned long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ unsigned long long ppred_wave_max(unsigned long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

template <bool PW>
__global__ void __launch_bounds__(kPpredBlock) ppred_kernel(const PpredArgs a) {
  __shared__ double sscale[PHT_PRED_MAXN];
  __shared__ double scum[PHT_PRED_MAXN * kPpredLd];
  __shared__ double sedges[PHT_PRED_MAXEDGES];
  __shared__ unsigned shist[PHT_PRED_MAXEDGES + 1];
  __shared__ unsigned long long stot[PHT_PRED_WORDS + 2]; /* the words, then ymin, ymax */
  const int tid = threadIdx.x, n = a.n, d = blockIdx.y, ne = a.ne;
  if (a.flags[d] != 0) return; /* flagged draw: the whole block, before any barrier */
  const int ld = n | 1;
  const unsigned long long kInfBits = 0x7ff0000000000000ull;
  pht_stage_math_tables();
  const double *tab = a.tab + (size_t)d * pht_pred_tab_words(n);
  for (int k = tid; k < n; k += kPpredBlock) sscale[k] = tab[k];
  for (int k = tid; k < n * n; k += kPpredBlock) scum[(k / n) * ld + (k % n)] = tab[n + k];
  for (int k = tid; k < ne; k += kPpredBlock) sedges[k] = a.edges[k];
  for (int k = tid; k <= ne; k += kPpredBlock) shist[k] = 0u;
  if (tid < PHT_PRED_WORDS + 2) stot[tid] = (tid == PHT_PRED_WORDS) ? kInfBits : 0ull;
  __syncthreads();

  const uint32_t stride = gridDim.x * (uint32_t)kPpredBlock; /* (< 2^32: the launcher bounds the grid) */
  uint32_t rep = blockIdx.x * (uint32_t)kPpredBlock + (uint32_t)tid;
  bool live = rep < a.nrep; /* a replicate in hand */
  bool fresh = true;        /* ... whose path has not started */
  pht_stream rs;
  int j = 0, nj = 0, oc = 0;
  bool ended = false;
  double t = 0.0;
  long long hy = 0, fy = 0, hq = 0, fq = 0, njump = 0;
  unsigned ndone = 0, nbad = 0, nsurv = 0;
  unsigned long long ymin = kInfBits, ymax = 0ull;

  while (__any(live)) {
    if (live && fresh) {
      pht_stream_init(&rs, a.k0, a.k1, a.rep0 + rep, PHT_PRED_TAG, a.draw0 + (uint32_t)d);
      j = 0;
      nj = 0;
      oc = 0;
      t = 0.0;
      ended = false;
      fresh = false;
    }
#pragma unroll
    for (int h = 0; h < kPpredJumps; h++) {
      if ((h & 1) == 0 && live) pht_stream_topup(&rs);
      if (live && !ended) {
        if (nj >= a.max_jumps) {
          oc = PHT_PRED_BAD;
          ended = true;
        } else {
          nj++;
          j = pht_pred_step(n, sscale, scum, ld, j, a.horizon, &rs, &t);
          if (j < 0) oc = PHT_PRED_SURV;
          ended = (j < 0) || (j == n);
        }
      }
    }
    if (live && ended) { /* record, then the stripe's next replicate */
      const double y = (oc & PHT_PRED_BAD) ? NAN : pht_pred_record(t, a.horizon, &oc);
      if (oc & PHT_PRED_BAD) {
        nbad++;
      } else {
        long long h1, f1, h2, f2;
        pht_ll_fixed(y, &h1, &f1);
        pht_ll_fixed(y * y, &h2, &f2);
        hy += h1;
        fy += f1;
        hq += h2;
        fq += f2;
        ndone++;
        nsurv += (oc & PHT_PRED_SURV) ? 1u : 0u;
        njump += nj;
        const unsigned long long yb = (unsigned long long)__double_as_longlong(y);
        ymin = yb < ymin ? yb : ymin;
        ymax = yb > ymax ? yb : ymax;
        atomicAdd(&shist[pht_pred_bin(sedges, ne, y)], 1u);
      }
      if (PW) {
        const size_t at = (size_t)d * (size_t)a.nrep + (size_t)rep;
        a.y[at] = (oc & PHT_PRED_BAD) ? NAN : y;
        a.nj[at] = nj;
      }
      rep += stride;
      live = rep < a.nrep;
      fresh = true;
    }
  }

  hy = wave_sum(hy);
  fy = wave_sum(fy);
  hq = wave_sum(hq);
  fq = wave_sum(fq);
  njump = wave_sum(njump);
  /* three counts of at most 2^22 per lane: 64 lanes of each fit 28 bits */
  const long long c01 = wave_sum((long long)ndone | ((long long)nbad << 32));
  const long long c2 = wave_sum((long long)nsurv);
  ymin = ppred_wave_min(ymin);
  ymax = ppred_wave_max(ymax);
  if ((tid & 63) == 0) {
    atomicAdd(stot + PHT_PRED_W_HY, (unsigned long long)hy);
    atomicAdd(stot + PHT_PRED_W_FY, (unsigned long long)fy);
    atomicAdd(stot + PHT_PRED_W_HQ, (unsigned long long)hq);
    atomicAdd(stot + PHT_PRED_W_FQ, (unsigned long long)fq);
    atomicAdd(stot + PHT_PRED_W_NDONE, (unsigned long long)(c01 & 0xffffffffll));
    atomicAdd(stot + PHT_PRED_W_NBAD, (unsigned long long)(c01 >> 32));
    atomicAdd(stot + PHT_PRED_W_NSURV, (unsigned long long)c2);
    atomicAdd(stot + PHT_PRED_W_NJUMP, (unsigned long long)njump);
    atomicMin(stot + PHT_PRED_WORDS, ymin);
    atomicMax(stot + PHT_PRED_WORDS + 1, ymax);
  }
  __syncthreads();
  if (tid < PHT_PRED_WORDS) {
    if (stot[tid] != 0ull) atomicAdd(a.words + (size_t)d * PHT_PRED_WORDS + tid, stot[tid]);
  } else if (tid == PHT_PRED_WORDS) {
    atomicMin(a.ymin + d, stot[PHT_PRED_WORDS]);
  } else if (tid == PHT_PRED_WORDS + 1) {
    atomicMax(a.ymax + d, stot[PHT_PRED_WORDS + 1]);
  }
  for (int k = tid; k <= ne; k += kPpredBlock)
    if (shist[k] != 0u) atomicAdd(a.counts + (size_t)d * (size_t)(ne + 1) + k, (unsigned long long)shist[k]);
}

}  // namespace pht

extern "C" hipError_t pht_launch_ppred(const pht::PpredArgs *a, int blocks_per_draw, hipStream_t st) {
  using namespace pht;
  if (!a || a->n < 1 || a->n > PHT_PRED_MAXN || a->nd < 1 || a->nd > kPpredBatch || a->nrep < 1 ||
      a->nrep > (uint32_t)PHT_PRED_MAXREP || a->max_jumps < 1 || a->max_jumps > PHT_PRED_MAXJUMPS || a->ne < 0 ||
      a->ne > PHT_PRED_MAXEDGES || !(a->horizon > 0.0) || !a->flags || !a->tab || (a->ne > 0 && !a->edges) ||
      !a->words || !a->ymin || !a->ymax || !a->counts || (!a->y != !a->nj) || blocks_per_draw < 1 ||
      blocks_per_draw > 65535)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks_per_draw, (unsigned)a->nd);
  if (a->y)
    hipLaunchKernelGGL((ppred_kernel<true>), grid, dim3(kPpredBlock), 0, st, *a);
  else
    hipLaunchKernelGGL((ppred_kernel<false>), grid, dim3(kPpredBlock), 0, st, *a);
  return hipGetLastError();
}
