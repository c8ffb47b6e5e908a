/*
 * pht_estep.hip — the expected sufficient statistics (E-step) of posterior
 * draws or EM iterates over a shard's resident observations (specification:
 * include/pht_estep.h).  The (ax, ac) tables are pht_loglik_unif.hip's
 * (pht_launch_llunif_table); two kernels of its own per batch of draws.
 *
 * estep_hist_kernel: one lane per observation over the context's sorted y,
 * tiles of 1024 strided over a capped grid (as llunif_kernel takes them: a
 * block sees small and large y alike; PHT_ESTEP_CONTIG gives each block one
 * contiguous range instead, which touches fewer bins but leaves the blocks
 * with the largest y, so the widest windows, to set the kernel's time: 188
 * against 120 us per draw).  A block walks the launch's draws
 * one after the other: the draw's table, invk and the draw's histogram
 * [class][k][G, T] live in LDS (32 + 16 + 64 KB at the cap K = 2047: one
 * block a CU).  Each lane evaluates its window (pht_es_window: the
 * log-likelihood's totals as in llunif_kernel), then runs the second pass over
 * its own window, k0 down to klo and then k0 + 1 up to khi in one loop, and
 * adds its words into the block's histogram with LDS atomics.  y is sorted, so
 * the lanes' windows nearly coincide: in lock step all 64 lanes of a wavefront
 * would hit one bin and the atomics would serialise 64 ways.  The lanes are
 * SKEWED instead: lane L starts (L & PHT_ESTEP_SKEW) steps late, so at most
 * four lanes with the same k0 meet on a bin at the default 15 (a wider skew
 * costs more idle steps than it saves conflicts: 7 and 15 measured the same,
 * 31 ten per cent slower, 63 more).  Conflicts cost time only: the sums are
 * integers.  PHT_ESTEP_WAVESUM builds the other design for the A/B: the
 * wavefront in step over absolute k, the words summed over the wave by
 * shuffles, one LDS add per wave, bin and word; with twelve dependent 64-bit
 * shuffle steps per k it took 500 us per draw.  At the end of a draw the block
 * flushes its non-zero bins with 64-bit atomics.  Integer sums: the result
 * does not depend on the grid.
 *
 * estep_contract_kernel: one workgroup per draw, one lane per cell (i, j);
 * R (both layouts), Hx, Hc and f in LDS (33 KB at n = 32), the accumulators
 * in registers; sequential in k, pht_es_contract's orders.
 */
#include <hip/hip_runtime.h>

#include "pht_estep.h"
#include "pht_estep_args.h"
#include "pht_kernels.h"
#include "pht_layout.h"
#include "pht_loglik_unif_args.h"
#include "pht_wave.h"

namespace pht {

#ifndef PHT_ESTEP_BLOCK
#define PHT_ESTEP_BLOCK 1024
#endif
constexpr int kEstepBlock = PHT_ESTEP_BLOCK;
static_assert(kEstepBlock % 64 == 0 && kEstepBlock >= 64 && kEstepBlock <= 1024, "whole waves");
/* the lanes' skew in the second pass: lane L is delayed by (L & kEstepSkew)
 * steps (63: lanes with one k0 never meet on a bin; 31, 15, 7: at most 2, 4, 8 do) */
#ifndef PHT_ESTEP_SKEW
#define PHT_ESTEP_SKEW 15
#endif
constexpr int kEstepSkew = PHT_ESTEP_SKEW;
static_assert(kEstepSkew >= 0 && kEstepSkew <= 63 && (kEstepSkew & (kEstepSkew + 1)) == 0, "a lane mask");
constexpr int kEstepCells = kMaxN * kMaxN;
static_assert(kMaxN == 32 && kEstepCells == 1024, "one lane per cell of a 32 x 32 generator");

__device__ __forceinline__ int es_wave_max(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ int es_wave_min(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
  return v;
}

/* one absolute k of the second pass: the wave's sums of the lanes' words into
 * the block's histogram (hasx / hasc: the wave holds a good lane of the class) */
__device__ __forceinline__ void es_emit(unsigned long long *shist, int k, long long g, long long t, int cens,
                                        bool hasx, bool hasc, bool lane0) {
  if (hasx) {
    const long long gs = wave_sum(cens ? 0ll : g), ts = wave_sum(cens ? 0ll : t);
    if (lane0 && (gs | ts)) {
      atomicAdd(shist + pht_es_idx(0, k, 0), (unsigned long long)gs);
      atomicAdd(shist + pht_es_idx(0, k, 1), (unsigned long long)ts);
    }
  }
  if (hasc) {
    const long long gs = wave_sum(cens ? g : 0ll), ts = wave_sum(cens ? t : 0ll);
    if (lane0 && (gs | ts)) {
      atomicAdd(shist + pht_es_idx(1, k, 0), (unsigned long long)gs);
      atomicAdd(shist + pht_es_idx(1, k, 1), (unsigned long long)ts);
    }
  }
}

__global__ void __launch_bounds__(kEstepBlock) estep_hist_kernel(const EstepHistArgs a) {
  __shared__ double stab[2 * PHT_ES_ROWS];
  __shared__ double sinvk[PHT_ES_ROWS];
  __shared__ unsigned long long shist[PHT_ES_WORDS];
  __shared__ unsigned long long stot[PHT_LL_TOT];
  const int tid = threadIdx.x;
  const bool lane0 = (tid & 63) == 0;
  pht_stage_math_tables();
  for (int k = tid; k < PHT_ES_ROWS; k += kEstepBlock) sinvk[k] = k ? 1.0 / (double)k : 0.0;
  for (int k = tid; k < PHT_ES_WORDS; k += kEstepBlock) shist[k] = 0ull;
#ifdef PHT_ESTEP_CONTIG
  /* this block's observations [lo, hi): one contiguous range of whole wavefronts */
  const long per = (((a.count + (long)gridDim.x - 1) / (long)gridDim.x) + 63L) & ~63L;
  const long lo = min((long)blockIdx.x * per, a.count), hi = min(lo + per, a.count), step = kEstepBlock;
#else
  /* this block's observations: tiles of kEstepBlock, strided over the grid */
  const long lo = (long)blockIdx.x * kEstepBlock, hi = a.count, step = (long)gridDim.x * kEstepBlock;
#endif

  for (int d = 0; d < a.nd; d++) {
    const double *m = a.meta + (size_t)d * PHT_LLU_META;
    if (__double_as_longlong(m[PHT_LLU_M_FLAG]) != 0) continue; /* unusable draw: the same for every lane */
    const int K = min(min((int)m[PHT_LLU_M_K], a.Kmax), a.stride / 2 - 1);
    const double mu = m[PHT_LLU_M_MU], abar_x = m[PHT_LLU_M_ABAR];
    __syncthreads(); /* the previous draw's flush is through */
    for (int k = tid; k < 2 * (K + 1); k += kEstepBlock) stab[k] = a.tab[(size_t)d * a.stride + k];
    if (tid < PHT_LL_TOT) stot[tid] = 0ull;
    __syncthreads();

    for (long base = lo; base < hi; base += step) {
      const long pos = base + tid;
      const bool live = pos < hi;
      const double y = live ? a.y[pos] : 1.0;
      const int cens = live ? (a.cens[pos] != 0) : 0;
      int bad;
      pht_es_win_t win;
      const double l = pht_es_window(stab, sinvk, K, mu, abar_x, y, cens, &bad, &win);
      long long h = 0, f = 0, bo = 0; /* bo: bad << 32 | obs */
      if (live) {
        if (bad) {
          bo = 1ll << 32;
        } else {
          pht_ll_fixed(l, &h, &f);
          bo = 1;
        }
      }
      h = wave_sum(h);
      f = wave_sum(f);
      bo = wave_sum(bo);
      if (lane0) {
        atomicAdd(stot + 0, (unsigned long long)h);
        atomicAdd(stot + 1, (unsigned long long)f);
        atomicAdd(stot + 2, (unsigned long long)(bo >> 32));
        atomicAdd(stot + 3, (unsigned long long)(bo & 0xffffffffll));
      }

      const bool good = live && !bad;
      const double *acol = stab + (cens ? 1 : 0);
      const double rn = 1.0 / win.num, yr = y * a.ryscale;
#ifndef PHT_ESTEP_WAVESUM
      /* the second pass over the lane's own window (every k in [klo, khi], so
       * in [0, K]), the lanes skewed so that few of them meet on a bin */
      const int lane = tid & 63;
      unsigned long long *hrow = shist + pht_es_idx(cens ? 1 : 0, 0, 0);
      const int delay = lane & kEstepSkew;
      const int cd = good ? win.k0 - win.klo + 1 : 0, cnt = good ? win.khi - win.klo + 1 : 0;
      const int T = es_wave_max(cnt ? delay + cnt : 0);
      double w = 1.0;
      for (int t = 0; t < T; t++) {
        const int j = t - delay;
        if (j >= 0 && j < cnt) {
          /* terms k0 .. klo, then k0 + 1 .. khi (w restarts from 1 at the mode) */
          const bool up = j >= cd;
          const int k = up ? win.k0 + 1 + (j - cd) : win.k0 - j;
          const double wp = (j == cd) ? 1.0 : w;
          w = up ? pht_es_up(wp, k, win.lam, sinvk) : ((j > 0) ? pht_es_down(wp, k + 1, win.il) : 1.0);
          long long g, tt;
          pht_es_word(w, acol[2 * k], rn, yr, &g, &tt);
          atomicAdd(hrow + 2 * k, (unsigned long long)g);
          atomicAdd(hrow + 2 * k + 1, (unsigned long long)tt);
        }
      }
#else
      /* the second pass, the wave in step over absolute k (every k below lies
       * in a good lane's window, so in [0, K]) */
      const int kdh = es_wave_max(good ? win.k0 : -1);
      if (kdh < 0) continue; /* no good lane in this wave */
      const bool hasx = __ballot(good && !cens) != 0ull, hasc = __ballot(good && cens) != 0ull;
      const int kdl = es_wave_min(good ? win.klo : 0x7fffffff);
      double w = 1.0;
      for (int k = kdh; k >= kdl; k--) {
        const bool in = good && k <= win.k0 && k >= win.klo;
        if (in && k < win.k0) w = pht_es_down(w, k + 1, win.il);
        long long g = 0, t = 0;
        if (in) pht_es_word(w, acol[2 * k], rn, yr, &g, &t);
        es_emit(shist, k, g, t, cens, hasx, hasc, lane0);
      }
      const int kul = es_wave_min(good ? win.k0 + 1 : 0x7fffffff), kuh = es_wave_max(good ? win.khi : -1);
      w = 1.0;
      for (int k = kul; k <= kuh; k++) {
        const bool in = good && k > win.k0 && k <= win.khi;
        long long g = 0, t = 0;
        if (in) {
          w = pht_es_up(w, k, win.lam, sinvk);
          pht_es_word(w, acol[2 * k], rn, yr, &g, &t);
        }
        es_emit(shist, k, g, t, cens, hasx, hasc, lane0);
      }
#endif
    }
    __syncthreads();
    /* flush the draw's non-zero bins (rows 0..K of both classes) and clear them */
    unsigned long long *gw = a.words + (size_t)d * PHT_ES_WORDS;
    for (int c = tid; c < 4 * (K + 1); c += kEstepBlock) {
      const int cls = c / (2 * (K + 1)), r = c - cls * 2 * (K + 1);
      const int li = cls * 2 * PHT_ES_ROWS + r;
      const unsigned long long v = shist[li];
      if (v != 0ull) {
        atomicAdd(gw + li, v);
        shist[li] = 0ull;
      }
    }
    if (tid < PHT_LL_TOT && stot[tid] != 0ull) atomicAdd(a.totals + (size_t)d * PHT_LL_TOT + tid, stot[tid]);
  }
}

__global__ void __launch_bounds__(kEstepCells) estep_contract_kernel(const EstepContractArgs a) {
  __shared__ double sR[kEstepCells];  /* [l][j] = R[l][j] */
  __shared__ double sRt[kEstepCells]; /* [l][j] = R[j][l] */
  __shared__ double sHx[kEstepCells], sHc[kEstepCells];
  __shared__ double sf[kMaxN], ss[kMaxN];
  __shared__ int sklast;
  const int d = blockIdx.x, tid = threadIdx.x, n = a.n;
  const bool cell = tid < n * n, vec = tid < n;
  const int i = cell ? tid / n : 0, j = cell ? tid - i * n : 0;
  const double *meta = a.meta + (size_t)d * PHT_LLU_META;
  const int no = n * n + 3 * n;
  double *out = a.out + (size_t)d * no;
  double *Z = out, *N = out + n, *E = out + n + n * n, *A = E + n;
  if (__double_as_longlong(meta[PHT_LLU_M_FLAG]) != 0) { /* flagged draw: the whole workgroup */
    if (tid < no) out[tid] = NAN;
    if (tid + kEstepCells < no) out[tid + kEstepCells] = NAN;
    return;
  }
  const int K = min((int)meta[PHT_LLU_M_K], a.stride / 2 - 1);
  const long long *words = a.words + (size_t)d * PHT_ES_WORDS;
  const double *tab = a.tab + (size_t)d * a.stride;
  const double *S = a.S + (size_t)d * n * n, *s = a.s + (size_t)d * n;
  const double rinv = 1.0 / meta[PHT_LLU_M_MU];
  if (tid == 0) sklast = -1;
  __syncthreads();
  for (int k = tid; k <= K; k += kEstepCells)
    if (words[pht_es_idx(0, k, 0)] | words[pht_es_idx(0, k, 1)] | words[pht_es_idx(1, k, 0)] |
        words[pht_es_idx(1, k, 1)])
      atomicMax(&sklast, k);
  if (cell) {
    const double r = pht_llu_R(S[i + j * n], rinv, i == j);
    sR[i * n + j] = r;
    sRt[j * n + i] = r;
    sHx[tid] = (i == 0) ? s[j] : 0.0;
    sHc[tid] = (i == 0) ? 1.0 : 0.0;
  }
  if (vec) {
    sf[tid] = (tid == 0) ? 1.0 : 0.0;
    ss[tid] = s[tid];
  }
  __syncthreads();
  const int klast = sklast;
  const double Rij = cell ? sR[tid] : 0.0;
  const double si = vec ? ss[tid] : 0.0, sj = cell ? ss[j] : 0.0;
  double acc = 0.0, eacc = 0.0, aacc = 0.0; /* Z_i on the diagonal cell, N_ij off it; E_tid, A_tid */
  for (int k = 0; k <= klast; k++) {
    double c[6];
    pht_es_coefs(words, k, K, a.yscale, tab[2 * k], tab[2 * k + 1], (k < K) ? tab[2 * k + 2] : 0.0,
                 (k < K) ? tab[2 * k + 3] : 0.0, c);
    if (cell) {
      const double hx = sHx[tid], hc = sHc[tid];
      if (i == j) {
        acc = fma(c[0], hx, acc);
        acc = fma(c[1], hc, acc);
      } else {
        acc = fma(c[2], Rij * hx, acc);
        acc = fma(c[3], Rij * hc, acc);
      }
    }
    if (vec) {
      const double fk = sf[tid];
      eacc = fma(c[4], fk * si, eacc);
      aacc = fma(c[5], fk, aacc);
    }
    if (k == klast) break;
    double fn = 0.0, x = 0.0, cc = 0.0;
    if (vec)
      for (int l = 0; l < n; l++) fn = fma(sf[l], sR[l * n + tid], fn);
    if (cell)
      for (int l = 0; l < n; l++) {
        const double r = sRt[l * n + j];
        x = fma(sHx[i * n + l], r, x);
        cc = fma(sHc[i * n + l], r, cc);
      }
    __syncthreads(); /* every lane has read f, Hx, Hc of step k */
    if (vec) sf[tid] = fn;
    __syncthreads();
    if (cell) {
      const double fi = sf[i];
      sHx[tid] = fma(fi, sj, x);
      sHc[tid] = fma(fi, 1.0, cc);
    }
    __syncthreads();
  }
  if (cell) {
    if (i == j)
      Z[i] = acc;
    N[i + j * n] = (i == j) ? 0.0 : acc;
  }
  if (vec) {
    E[tid] = eacc;
    A[tid] = aacc;
  }
}

}  // namespace pht

extern "C" hipError_t pht_launch_estep_hist(const pht::EstepHistArgs *a, int grid_cap, hipStream_t st) {
  using namespace pht;
  if (!a || a->nd < 1 || a->nd > kLoglikBatch || a->count < 1 || !a->y || !a->cens || !a->meta || !a->tab ||
      !a->totals || !a->words || grid_cap < 1 || a->Kmax < 0 || a->Kmax > PHT_LLU_MAXK ||
      a->stride < 2 * (a->Kmax + 1) || !(a->ryscale > 0.0))
    return hipErrorInvalidValue;
  const long tiles = (a->count + kEstepBlock - 1) / kEstepBlock;
  const int grid = (int)(tiles < (long)grid_cap ? tiles : (long)grid_cap);
  hipLaunchKernelGGL(estep_hist_kernel, dim3(grid), dim3(kEstepBlock), 0, st, *a);
  return hipGetLastError();
}

extern "C" hipError_t pht_launch_estep_contract(const pht::EstepContractArgs *a, hipStream_t st) {
  using namespace pht;
  if (!a || a->n < 1 || a->n > kMaxN || a->nd < 1 || a->nd > kLoglikBatch || !a->S || !a->s || !a->meta || !a->tab ||
      !a->words || !a->out || a->stride < 2 || a->stride > 2 * (PHT_LLU_MAXK + 1) || !(a->yscale > 0.0))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(estep_contract_kernel, dim3(a->nd), dim3(kEstepCells), 0, st, *a);
  return hipGetLastError();
}
