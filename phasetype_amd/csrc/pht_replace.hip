/*
 * pht_replace.hip — age-replacement policies of posterior draws
 * (specification: include/pht_replace.h).  The (ax, ac) tables are
 * pht_loglik_unif.hip's (pht_launch_llunif_table); two kernels of its own per
 * batch of draws.
 *
 * rp_curve_kernel: one lane per (draw, age).  A block of 256 lanes first
 * stages, for each of its draws, the draw's table (32 KB at the cap K = 2047)
 * and once 1 / k (16 KB) in LDS, then one lane per draw sums the survival
 * column into the draw's prefix sums cc (16 KB at the cap, pht_rp_cc) beside
 * the table; the blocks of the first tile write cc out for the policy kernel.
 * After that barrier every lane evaluates lS, lf and M at its age.  Packing
 * (pht_replace_pack) as the quantile kernel's, with one pool: a slot at the cap
 * is 48 KB, 71 KB a block with 1 / k and the math tables, two blocks a CU.
 *
 * rp_policy_kernel: one wavefront per (draw, cost pair); a block of four
 * waves takes four pairs of one draw and stages the draw's table, cc and 1 / k
 * once (the same 71 KB).  The lanes stride over the curve for the argmin (a
 * wave minimum, the lowest index on ties); every multisection step of
 * pht_rp_policy puts its 64 points into the 64 lanes and finds the sign change
 * by ballot.  Lane 0 writes the seven words.
 */
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pht_kernels.h"
#include "pht_layout.h"
#include "pht_loglik_unif_args.h"
#include "pht_replace.h"
#include "pht_replace_args.h"

namespace pht {

static_assert(kRpRows == PHT_LLU_MAXK + 1, "a table at the cap");
static_assert(kRpBlock % 64 == 0 && kRpBlock >= 64 && kRpBlock <= 1024, "whole waves");
static_assert(PHT_RP_NPT == 64, "a multisection step is one wavefront");

__global__ void __launch_bounds__(kRpBlock) rp_curve_kernel(const ReplaceCurveArgs a) {
  __shared__ double spool[3 * kRpRows];
  __shared__ double sinvk[kRpRows];
  const int tid = threadIdx.x;
  const int rows = a.Kmax + 1, slot = 3 * rows;
  const int dbase = blockIdx.x * a.dpb;
  pht_stage_math_tables();
  for (int k = tid; k <= a.Kmax; k += kRpBlock) sinvk[k] = k ? 1.0 / (double)k : 0.0;
  for (int g = 0; g < a.dpb && dbase + g < a.nd; g++) {
    const int d = dbase + g;
    const double *m = a.meta + (size_t)d * PHT_LLU_META;
    if (__double_as_longlong(m[PHT_LLU_M_FLAG]) != 0) continue; /* flagged draw: no table */
    const int K = min((int)m[PHT_LLU_M_K], a.Kmax);
    for (int k = tid; k < 2 * (K + 1); k += kRpBlock) spool[g * slot + k] = a.tab[(size_t)d * a.stride + k];
  }
  __syncthreads();
  if (tid < a.dpb && dbase + tid < a.nd) { /* the draw's prefix sums, once per draw */
    const double *m = a.meta + (size_t)(dbase + tid) * PHT_LLU_META;
    if (__double_as_longlong(m[PHT_LLU_M_FLAG]) == 0)
      pht_rp_cc(spool + tid * slot, min((int)m[PHT_LLU_M_K], a.Kmax), spool + tid * slot + 2 * rows);
  }
  __syncthreads();
  if (blockIdx.y == 0) {
    for (int g = 0; g < a.dpb && dbase + g < a.nd; g++) {
      const int d = dbase + g;
      const double *m = a.meta + (size_t)d * PHT_LLU_META;
      if (__double_as_longlong(m[PHT_LLU_M_FLAG]) != 0) continue;
      const int K = min((int)m[PHT_LLU_M_K], a.Kmax);
      for (int k = tid; k <= K; k += kRpBlock) a.cc[(size_t)d * a.ccstride + k] = spool[g * slot + 2 * rows + k];
    }
  }

  const int g = tid / a.lp, i = tid - g * a.lp;
  const int d = dbase + g;
  const long ai = (long)blockIdx.y * kRpBlock + i;
  if (g >= a.dpb || d >= a.nd || ai >= (long)a.G) return; /* no barrier below */
  const double *m = a.meta + (size_t)d * PHT_LLU_META;
  double lS = NAN, lf = NAN, M = NAN;
  unsigned fl = PHT_RP_A_DRAW;
  if (__double_as_longlong(m[PHT_LLU_M_FLAG]) == 0)
    fl = pht_rp_curve(spool + g * slot, spool + g * slot + 2 * rows, sinvk, min((int)m[PHT_LLU_M_K], a.Kmax),
                      m[PHT_LLU_M_MU], m[PHT_LLU_M_ABAR], a.thi[d], a.ages[ai], &lS, &lf, &M);
  const size_t at = (size_t)d * (size_t)a.G + (size_t)ai;
  a.lS[at] = lS;
  a.lf[at] = lf;
  a.M[at] = M;
  a.aflags[at] = fl;
}

/* (g, index) of the better of two candidates: the smaller g, the lower index
 * on a tie; an index < 0 is no candidate */
__device__ __forceinline__ void rp_better(double &g, int &j, double og, int oj) {
  if (oj >= 0 && (j < 0 || og < g || (og == g && oj < j))) {
    g = og;
    j = oj;
  }
}

__global__ void __launch_bounds__(kRpBlock) rp_policy_kernel(const ReplacePolicyArgs a) {
  __shared__ double stab[2 * kRpRows];
  __shared__ double scc[kRpRows];
  __shared__ double sinvk[kRpRows];
  const int tid = threadIdx.x, lane = tid & 63;
  const int d = blockIdx.x;
  const int p = blockIdx.y * kRpWaves + (tid >> 6);
  const double *m = a.meta + (size_t)d * PHT_LLU_META;
  const bool flagged = __double_as_longlong(m[PHT_LLU_M_FLAG]) != 0;
  const int K = flagged ? 0 : min((int)m[PHT_LLU_M_K], a.Kmax);
  pht_stage_math_tables();
  if (!flagged) {
    for (int k = tid; k <= K; k += kRpBlock) sinvk[k] = k ? 1.0 / (double)k : 0.0;
    for (int k = tid; k < 2 * (K + 1); k += kRpBlock) stab[k] = a.tab[(size_t)d * a.stride + k];
    for (int k = tid; k <= K; k += kRpBlock) scc[k] = a.cc[(size_t)d * a.ccstride + k];
  }
  __syncthreads();
  if (p >= a.P) return; /* whole waves; no barrier below */

  const size_t at = (size_t)d * (size_t)a.P + (size_t)p;
  pht_rp_out_t o;
  const double cp = a.cp[p], cf = a.cf[p];
  const double mu = m[PHT_LLU_M_MU], abar = m[PHT_LLU_M_ABAR];
  const double *ages = a.ages;
  const double *lS = a.lS + (size_t)d * a.G, *lf = a.lf + (size_t)d * a.G, *M = a.M + (size_t)d * a.G;
  const unsigned *af = a.aflags + (size_t)d * a.G;
  bool done = false;
  if (flagged) {
    pht_rp_flagged(&o);
    done = true;
  } else if (!pht_rp_cost_ok(cp, cf)) {
    pht_rp_set(&o, NAN, NAN, NAN, NAN, -1, 0, PHT_RP_F_COST);
    done = true;
  }
  if (!done) {
    /* 1. the grid's argmin over the wave */
    int j = -1, jlast = -1;
    double gj = INFINITY;
    for (int i = lane; i < a.G; i += 64) {
      if (af[i]) continue;
      const double g = pht_rp_gsel(lS[i], M[i], cp, cf);
      jlast = i;
      rp_better(gj, j, g, i);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double og = __shfl_xor(gj, off, 64);
      const int oj = __shfl_xor(j, off, 64);
      const int ol = __shfl_xor(jlast, off, 64);
      rp_better(gj, j, og, oj);
      jlast = max(jlast, ol);
    }
    if (j < 0) {
      pht_rp_set(&o, NAN, NAN, NAN, NAN, -1, 0, PHT_RP_F_NOAGE);
      done = true;
    } else {
      const double ginf = cf / a.mean[d], c0 = pht_rp_c0(cp, cf);
      /* 2. the bracket (the same words in every lane) */
      double lo, hi;
      unsigned fl;
      if (!pht_rp_bracket(a.G, ages, lS, lf, M, af, j, jlast, c0, &lo, &hi, &fl)) {
        pht_rp_finish(&o, ages[j], gj, ages[j], ages[j], j, 0, fl, ginf);
        done = true;
      }
      /* 3. the refinement: a step's 64 points in the 64 lanes */
      int nev = 0, step = 0, bad;
      while (!done && !pht_rp_stop(lo, hi)) {
        if (step >= PHT_RP_MAXSTEP) {
          pht_rp_set(&o, NAN, NAN, lo, hi, j, nev, PHT_RP_F_CAP);
          done = true;
          break;
        }
        step++;
        if (__all(pht_rp_inside_i(lo, hi, lane + 1))) {
          const double dv = pht_rp_D_at(stab, scc, sinvk, K, mu, abar, pht_rp_point(lo, hi, lane + 1), c0, &bad);
          nev += PHT_RP_NPT;
          if (__any(bad)) {
            pht_rp_set(&o, NAN, NAN, lo, hi, j, nev, PHT_RP_F_EVAL);
            done = true;
            break;
          }
          const unsigned long long mask = __ballot(dv >= 0.0);
          const int first = mask ? __ffsll((long long)mask) : 0; /* 1-based: the point's number */
          const double na = pht_rp_point(lo, hi, first ? first - 1 : PHT_RP_NPT);
          const double nb = first ? pht_rp_point(lo, hi, first) : hi;
          lo = na;
          hi = nb;
        } else {
          const double t = pht_q_mid(lo, hi);
          const double dv = pht_rp_D_at(stab, scc, sinvk, K, mu, abar, t, c0, &bad);
          nev++;
          if (bad) {
            pht_rp_set(&o, NAN, NAN, lo, hi, j, nev, PHT_RP_F_EVAL);
            done = true;
            break;
          }
          if (dv >= 0.0)
            hi = t;
          else
            lo = t;
        }
      }
      /* 4. and 5. */
      if (!done) {
        double th = lo + 0.5 * (hi - lo);
        th = (th < lo) ? lo : ((th > hi) ? hi : th);
        double l1, l2, mm;
        int khi;
        bad = pht_rp_eval3(stab, scc, sinvk, K, mu, abar, th, &l1, &l2, &mm, &khi);
        nev++;
        if (bad)
          pht_rp_set(&o, NAN, NAN, lo, hi, j, nev, PHT_RP_F_EVAL);
        else
          pht_rp_finish(&o, th, pht_rp_g(l1, mm, cp, cf), lo, hi, j, nev, 0u, ginf);
      }
    }
  }
  if (lane == 0) {
    a.t[at] = o.t;
    a.g[at] = o.g;
    a.lo[at] = o.lo;
    a.hi[at] = o.hi;
    a.j[at] = o.j;
    a.nev[at] = o.nev;
    a.flags[at] = o.flags;
  }
}

}  // namespace pht

extern "C" int pht_replace_pack(int nd, int G, int Kmax) {
  using namespace pht;
  const int lp = G < kRpBlock ? G : kRpBlock;
  const int want = std::min(kRpBlock / lp, nd), fit = kRpRows / (Kmax + 1);
  return std::max(1, std::min(want, fit));
}

extern "C" hipError_t pht_launch_replace_curve(const pht::ReplaceCurveArgs *a, hipStream_t st) {
  using namespace pht;
  if (!a || a->nd < 1 || a->nd > kLoglikBatch || a->G < 1 || a->G > PHT_RP_MAXG || !a->meta || !a->thi || !a->tab ||
      !a->ages || !a->cc || !a->lS || !a->lf || !a->M || !a->aflags || a->Kmax < 0 || a->Kmax > PHT_LLU_MAXK ||
      a->stride < 2 * (a->Kmax + 1) || a->ccstride < a->Kmax + 1)
    return hipErrorInvalidValue;
  const int dpb = pht_replace_pack(a->nd, a->G, a->Kmax);
  /* the launch's packing must be the rule's: the LDS slots are sized by it */
  if (a->dpb != dpb || a->lp != (a->G < kRpBlock ? a->G : kRpBlock)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a->nd + dpb - 1) / dpb), (unsigned)((a->G + kRpBlock - 1) / kRpBlock));
  if (dpb > 1 && grid.y != 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rp_curve_kernel, grid, dim3(kRpBlock), 0, st, *a);
  return hipGetLastError();
}

extern "C" hipError_t pht_launch_replace_policy(const pht::ReplacePolicyArgs *a, hipStream_t st) {
  using namespace pht;
  if (!a || a->nd < 1 || a->nd > kLoglikBatch || a->G < 1 || a->G > PHT_RP_MAXG || a->P < 1 || a->P > PHT_RP_MAXP ||
      !a->meta || !a->mean || !a->tab || !a->cc || !a->ages || !a->lS || !a->lf || !a->M || !a->aflags || !a->cp ||
      !a->cf || !a->t || !a->g || !a->lo || !a->hi || !a->j || !a->nev || !a->flags || a->Kmax < 0 ||
      a->Kmax > PHT_LLU_MAXK || a->stride < 2 * (a->Kmax + 1) || a->ccstride < a->Kmax + 1)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)a->nd, (unsigned)((a->P + kRpWaves - 1) / kRpWaves));
  hipLaunchKernelGGL(rp_policy_kernel, grid, dim3(kRpBlock), 0, st, *a);
  return hipGetLastError();
}
