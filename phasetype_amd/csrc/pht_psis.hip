/*
 * pht_psis.hip — PSIS-LOO of the context's observations from the pointwise
 * log-likelihood matrix kept on the device (specification:
 * include/pht_psis.h; no reference counterpart).
 *
 * psis_transpose_kernel: a chunk of observations of the matrix
 * [draw][observation], usable rows only (the host's list), through a padded
 * 32 x 32 LDS tile into [observation][usable draw], so that a wavefront's
 * reads of one observation's draws are contiguous.
 *
 * psis_obs_kernel: one wavefront (= one block) per observation, striding over
 * the chunk; the math tables are staged once per block.  The observation's S
 * values are re-read from L2 / L1 for each pass, never held:
 *   NaN test, max of -l and of l; lppd's sum;
 *   the cutoff c = the (M + 1)-th largest weight by an exact radix select over
 *   the bits of |lw| (lw <= 0: ascending bits = descending lw), eight passes
 *   of eight bits with a 256-bin LDS histogram;
 *   the values above c into LDS (ballot offsets), filled up with copies of c,
 *   padded with +inf to a power of two and ordered there by a bitonic network
 *   (M <= 384: at most 512 slots; the S draws are never sorted);
 *   the fit: grid point j belongs to lane j - 1 (G <= 49), each lane runs its
 *   own sequential sum over the tail read from LDS as a broadcast, then its
 *   weight over the G values of L; theta_hat, k, sigma and khat are computed
 *   by every lane alike (sequential sums over LDS broadcasts);
 *   the smoothed tail, one lane per r; the largest terms, then lane p's
 *   partial sums over the positions = p (mod 64) and the xor butterfly.
 * Every barrier is reached by all 64 lanes: a block is one wavefront and all
 * branches around barriers are wave-uniform; lanes past an end are masked.
 */
#include <hip/hip_runtime.h>

#include "pht_psis.h"
#include "pht_psis_args.h"
#include "pht_wave.h"

namespace pht {

constexpr int kPsisTile = 32;
constexpr int kPsisTileRows = 8;
constexpr int kPsisSlots = 512; /* the power of two above PHT_PSIS_MAXM */
static_assert(kPsisSlots >= PHT_PSIS_MAXM, "the bitonic network holds the longest tail");
static_assert(PHT_PSIS_MAXG <= 64, "one lane per grid point");

__global__ void __launch_bounds__(kPsisTile *kPsisTileRows) psis_transpose_kernel(const PsisTransposeArgs a) {
  __shared__ double tile[kPsisTile][kPsisTile + 1];
  const int tx = threadIdx.x, ty = threadIdx.y;
  const long kb = (long)blockIdx.x * kPsisTile;
  const int ub = (int)blockIdx.y * kPsisTile;
#pragma unroll
  for (int r = 0; r < kPsisTile; r += kPsisTileRows) {
    const int u = ub + ty + r;
    const long k = kb + tx;
    if (u < a.S && k < a.kc) tile[ty + r][tx] = a.mat[(size_t)a.rows[u] * (size_t)a.count + (size_t)(a.k0 + k)];
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kPsisTile; r += kPsisTileRows) {
    const long k = kb + ty + r;
    const int u = ub + tx;
    if (k < a.kc && u < a.S) a.out[(size_t)k * (size_t)a.S + (size_t)u] = tile[tx][ty + r];
  }
}

__device__ __forceinline__ double psis_wave_max(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

__global__ void __launch_bounds__(64) psis_obs_kernel(const PsisArgs a) {
  __shared__ unsigned hist[256];
  __shared__ double stail[kPsisSlots];
  __shared__ double sx[PHT_PSIS_MAXM];
  __shared__ double ssm[PHT_PSIS_MAXM];
  __shared__ double sL[64];
  __shared__ double stw[64];
  const int lane = threadIdx.x;
  const int S = a.S;
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  const int M = pht_psis_tail_len(S);
  const int G = pht_psis_grid(M > 0 ? M : 1);
  int P = 8;
  while (P < M) P <<= 1;
  pht_stage_math_tables();
  __syncthreads();

  for (long obs = blockIdx.x; obs < a.kc; obs += gridDim.x) {
    const double *row = a.lt + (size_t)obs * (size_t)S;
    /* NaN test and the two maxima */
    bool isnan_ = false;
    double mx = -INFINITY, ml = -INFINITY;
    for (int d = lane; d < S; d += 64) {
      const double v = row[d];
      isnan_ = isnan_ || (v != v);
      mx = fmax(mx, -v);
      ml = fmax(ml, v);
    }
    if (__any(isnan_)) { /* wave-uniform */
      if (lane == 0) {
        a.elpd[obs] = NAN;
        a.khat[obs] = NAN;
        a.lppd[obs] = NAN;
        a.flags[obs] = PHT_PSIS_F_BAD;
      }
      continue;
    }
    mx = psis_wave_max(mx);
    ml = psis_wave_max(ml);
    double acc = 0.0;
    for (int d = lane; d < S; d += 64) acc = acc + pht_exp(row[d] - ml);
    const double lppd = (ml + pht_log(wave_sum(acc))) - pht_log((double)S);

    int fl = 0, ntie = 0;
    bool smooth = false;
    double c = 0.0, kh = INFINITY, sg = 0.0;
    if (M < 5) {
      fl = PHT_PSIS_F_SHORT;
    } else {
      /* the (M + 1)-th smallest |lw|: rank kk (from 0) among the keys */
      unsigned long long pref = 0ull;
      int kk = M;
      for (int shift = 56; shift >= 0; shift -= 8) {
        for (int b = lane; b < 256; b += 64) hist[b] = 0u;
        __syncthreads();
        const unsigned long long himask = (shift == 56) ? 0ull : (~0ull << (shift + 8));
        for (int d = lane; d < S; d += 64) {
          const unsigned long long key = pht_d2u((-row[d]) - mx) & 0x7fffffffffffffffull;
          if ((key & himask) == pref) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        const unsigned h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
        const int s4 = (int)(h0 + h1 + h2 + h3);
        int incl = s4;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const int o = __shfl_up(incl, off, 64);
          if (lane >= off) incl += o;
        }
        int cum = incl - s4, mydig = -1, mykk = 0;
        const unsigned hq[4] = {h0, h1, h2, h3};
#pragma unroll
        for (int q = 0; q < 4; q++) {
          if (mydig < 0 && kk >= cum && kk < cum + (int)hq[q]) {
            mydig = 4 * lane + q;
            mykk = kk - cum;
          }
          cum += (int)hq[q];
        }
        const unsigned long long hit = __ballot(mydig >= 0); /* exactly one lane */
        const int src = __ffsll((long long)hit) - 1;
        const int dig = __shfl(mydig, src, 64);
        kk = __shfl(mykk, src, 64);
        pref |= (unsigned long long)dig << shift;
        __syncthreads();
      }
      c = 0.0 - pht_u2d(pref);
      const double ec = pht_exp(c);
      /* the values above c, then copies of c, then the padding */
      int cg = 0;
      for (int d0 = 0; d0 < S; d0 += 64) {
        const int d = d0 + lane;
        const double lw = (d < S) ? (-row[d]) - mx : -INFINITY;
        const bool gt = (d < S) && (lw > c);
        const unsigned long long bal = __ballot(gt);
        const int at = cg + __popcll(bal & lt_mask); /* < M: at most M values exceed c */
        if (gt && at < kPsisSlots) stail[at] = lw;
        cg += __popcll(bal);
      }
      ntie = M - cg;
      for (int i = cg + lane; i < P; i += 64) stail[i] = (i < M) ? c : INFINITY;
      __syncthreads();
      for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int i = lane; i < P; i += 64) {
            const int ixj = i ^ j;
            if (ixj > i) {
              const double lo = stail[i], hi = stail[ixj];
              const bool up = (i & k) == 0;
              if (up ? (lo > hi) : (lo < hi)) {
                stail[i] = hi;
                stail[ixj] = lo;
              }
            }
          }
          __syncthreads();
        }
      for (int i = lane; i < M; i += 64) sx[i] = pht_exp(stail[i]) - ec;
      __syncthreads();
      if (sx[M - 1] == sx[0]) {
        fl = PHT_PSIS_F_CONST;
      } else {
        const double xmax = sx[M - 1], xs = sx[pht_psis_xs_index(M)];
        double th = 0.0;
        bool thbad = false;
        if (lane < G) {
          th = pht_psis_theta(G, lane + 1, xmax, xs);
          thbad = !(fabs(th) < INFINITY);
          sL[lane] = pht_psis_L(M, th, pht_psis_prof(th, sx, M));
        }
        __syncthreads();
        if (lane < G) stw[lane] = th * pht_psis_weight(G, sL, lane);
        __syncthreads();
        double theta_hat = 0.0;
        for (int j = 0; j < G; j++) theta_hat = theta_hat + stw[j];
        const int ok = pht_psis_fit_finish(M, theta_hat, sx, &kh, &sg) && !__any(thbad);
        if (!ok) {
          fl = PHT_PSIS_F_FIT;
          kh = INFINITY;
        } else {
          smooth = true;
          for (int r = 1 + lane; r <= M; r += 64) ssm[r - 1] = pht_psis_smoothed(r, M, kh, sg, ec);
        }
        __syncthreads();
      }
    }
    /* the two sums of elpd: the largest terms, then the partial sums */
    double ma = -INFINITY, mb = -INFINITY, pa = 0.0, pb = 0.0;
    for (int pass = 0; pass < 2; pass++) {
      int seen = 0;
      for (int d0 = 0; d0 < S; d0 += 64) {
        const int d = d0 + lane;
        const bool live = d < S;
        const double lw = live ? (-row[d]) - mx : -INFINITY;
        const bool eq = live && smooth && (lw == c);
        const unsigned long long bal = __ballot(eq);
        const bool skip = !live || (smooth && (lw > c || (eq && seen + __popcll(bal & lt_mask) < ntie)));
        seen += __popcll(bal);
        if (!skip) {
          const double b = lw, t = lw - (lw + mx);
          if (pass == 0) {
            ma = fmax(ma, t);
            mb = fmax(mb, b);
          } else {
            pa = pa + pht_exp(t - ma);
            pb = pb + pht_exp(b - mb);
          }
        }
      }
      if (smooth)
        for (int r = lane; r < M; r += 64) {
          const double b = ssm[r], t = ssm[r] - (stail[r] + mx);
          if (pass == 0) {
            ma = fmax(ma, t);
            mb = fmax(mb, b);
          } else {
            pa = pa + pht_exp(t - ma);
            pb = pb + pht_exp(b - mb);
          }
        }
      if (pass == 0) {
        ma = psis_wave_max(ma);
        mb = psis_wave_max(mb);
      }
    }
    const double elpd = (ma + pht_log(wave_sum(pa))) - (mb + pht_log(wave_sum(pb)));
    if (lane == 0) {
      a.elpd[obs] = elpd;
      a.khat[obs] = kh;
      a.lppd[obs] = lppd;
      a.flags[obs] = fl;
    }
    __syncthreads(); /* the LDS arrays are free for the next observation */
  }
}

}  // namespace pht

extern "C" hipError_t pht_launch_psis_transpose(const pht::PsisTransposeArgs *a, hipStream_t st) {
  using namespace pht;
  if (!a || !a->mat || !a->rows || !a->out || a->S < 1 || a->S > PHT_PSIS_MAXS || a->kc < 1 || a->k0 < 0 ||
      a->k0 + a->kc > a->count)
    return hipErrorInvalidValue;
  const long gx = (a->kc + kPsisTile - 1) / kPsisTile;
  if (gx > 0x7fffffffl) return hipErrorInvalidValue;
  const dim3 grid((unsigned)gx, (unsigned)((a->S + kPsisTile - 1) / kPsisTile));
  hipLaunchKernelGGL(psis_transpose_kernel, grid, dim3(kPsisTile, kPsisTileRows), 0, st, *a);
  return hipGetLastError();
}

extern "C" hipError_t pht_launch_psis(const pht::PsisArgs *a, int grid_cap, hipStream_t st) {
  using namespace pht;
  if (!a || !a->lt || !a->elpd || !a->khat || !a->lppd || !a->flags || a->S < 1 || a->S > PHT_PSIS_MAXS ||
      a->kc < 1 || grid_cap < 1)
    return hipErrorInvalidValue;
  const int grid = (int)(a->kc < (long)grid_cap ? a->kc : (long)grid_cap);
  hipLaunchKernelGGL(psis_obs_kernel, dim3(grid), dim3(64), 0, st, *a);
  return hipGetLastError();
}
