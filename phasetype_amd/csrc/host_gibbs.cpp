/*
 * host_gibbs.cpp — the reference's Gibbs bookkeeping and loop on the host
 * (src/PHT_MCMC_Aslett.c:187-405) over the contexts' sweeps, pht_gibbs_run
 * and the draw -> generator map.
 */
#include <math.h>

#include <cmath>

#include "host_internal.h"

using namespace pht;
using namespace pht::host;

/* fixed-point exponent for z: 52 - e with sum(y) < 2^e
 * (frexp), so the exact-observation total stays below 2^52 whatever the
 * time scale of the data (11 bits of int64 headroom are left for censored
 * paths running past y).  Clamped so 2^zexp is a finite normal double;
 * an empty, zero or non-finite sum gives 52. */
extern "C" int pht_zexp(const double *y, long l) {
  double sy = 0.0;
  for (long i = 0; i < l; i++) sy += y[i];
  if (!(sy > 0.0) || !std::isfinite(sy)) return 52;
  int e = 0;
  (void)frexp(sy, &e);
  return std::min(1000, std::max(-1000, 52 - e));
}

/* Run the Gibbs loop over a set of device shards; reduce = optional
 * cross-process all-reduce of the int64 statistics block. */
template <class Rng>
int pht::host::gibbs_run(Rng &R, int it, int method, int n, int m, const double *nu, const double *zeta, const int *T,
                         const double *C, int silent, const double *start, double *res, std::vector<pht_ctx *> &ctxs,
                         uint32_t k0, uint32_t k1, int zexp, pht_reduce_fn reduce, void *reduce_user,
                         double *kernel_ms_total) {
  ParamLists L;
  if (L.build(n, m, T, C)) {
    char why[160];
    L.describe(why, sizeof why);
    set_err("Gibbs run: %s", why);
    return -1;
  }
  GibbsState G(R, it, n, m, nu, zeta, T, L, start, res);
  OneBlasThread one; /* the per-sweep eigensystems on this thread */
  const int disp = dispatch_method(method);
  const int sl = stats_len(n);
  std::vector<long long> tot(sl);
  std::vector<double> z(n);
  std::vector<unsigned char> pb;
  say("Starting phase-type MCMC sampler ...\n\nBegining processing ...");
  if (silent) say(" silent processing selected, there will be no further feedback until MCMC run complete");
  /* kernel time: the sweeps' events on one sweep in `every` (the last of
   * each group, so a fresh chain's first and slowest sweeps do not weigh
   * more than their share; PHT_KTIME_EVERY, default 4, 1 = every sweep; the
   * last sweep when no other was timed), the total scaled from their mean;
   * chain groups time every sweep */
  const int every = std::max(1, env_int("PHT_KTIME_EVERY", 4));
  auto want_time = [&](int k) { return k % every == 0 || (k == it - 1 && k - 1 < every); };
  double kms = 0.0;
  long ktimed = 0;
  long long flagged = 0;
  /* Pipelined loop (contexts not in a chains group, not UNIF, whose enqueue
   * reads the parameters): sweep k + 1 is enqueued as soon as sweep k is,
   * behind a gate kernel per context that waits for its parameters, so the
   * launch work runs while sweep k does and only the Gamma update and the
   * next parameter block stay between two sweeps (PHT_PIPELINE=0: off).  The
   * draws are the same: sweep k + 1's parameters are those the update
   * produced from sweep k's statistics. */
  for (pht_ctx *c : ctxs)
    if (!c->grp) ctx_drain(c);
  bool pipe = !ctxs.empty() && it > 2;
  for (pht_ctx *c : ctxs) pipe = pipe && !c->grp && c->h_gate && c->method != kMethodUNIF && !c->ulaw;
  bool pending = false;                        /* every context holds a gated sweep */
  std::vector<unsigned> pgate(ctxs.size(), 0u); /* its gate (0: none enqueued) */
  /* an early return with gated sweeps enqueued: release them (they run on
   * the last staged parameters) and drain the streams, so nothing waits on
   * a gate */
  auto unwind = [&]() {
    for (size_t i = 0; i < ctxs.size(); i++) {
      if (pgate[i]) {
        ctx_release(ctxs[i], pgate[i], nullptr, 0);
        (void)hipStreamSynchronize(ctxs[i]->stream.get());
        ctxs[i]->nin = 0;
        pgate[i] = 0u;
      }
    }
    pending = false;
  };
  int first_flagged = 0;
  /* every sweep must account for every observation of every shard: the
   * node-wide processed count (extra word kXObs, after the reduce) is checked
   * against it, so a launch-shape bug that drops observations, or a reduce
   * that sums a block twice or not at all, fails the run instead of biasing
   * the posterior.  Multi-process: the count comes from
   * pht_ctx_set_global_count (unchecked when it was not given). */
  long long expect = 0;
  {
    bool multi = reduce != nullptr;
    for (pht_ctx *c : ctxs) {
      expect += c->count;
      multi = multi || c->comm != nullptr;
    }
    if (multi) expect = ctxs.size() == 1 ? ctxs[0]->global_count : -1;
  }
  /* the observed times alone must fit the fixed point with room to spare */
  for (pht_ctx *c : ctxs) {
    if (!(ldexp(c->ysum, zexp) < 0x1p62)) {
      set_err("zexp = %d overflows the fixed-point z sums: the shard's observed times total %g (pht_zexp gives %d)",
              zexp, c->ysum, pht_zexp(c->h_ysorted.data(), (long)c->h_ysorted.size()));
      return -1;
    }
  }
  for (int iter = 1; iter < it; iter++) {
    if (!silent) say("\rProcessing iteration %d of %d (%.1lf%%)\r", iter + 1, it, (100.0 * (iter + 1)) / it);
    if (!disp) {
      say("CRITICAL ERROR: Unknown sampling method (code = %d)\n\n", method);
      continue;
    }
    /* bridge contexts run the UNIF kernels: their block needs no eigensystem */
    const int bm = ctxs[0]->ulaw ? kMethodUNIF : (disp == kMethodMHRS ? kMethodMHRS : method);
    const int info = build_params(n, G.S.data(), G.s.data(), bm, pb);
    if (info < 0) {
      unwind();
      return -1;
    }
    const bool timed = want_time(iter);
    if (pending) {
      for (size_t i = 0; i < ctxs.size(); i++) {
        memcpy(ctxs[i]->h_params.get(), pb.data(), pb.size());
        ctx_release(ctxs[i], pgate[i], pb.data(), pb.size());
        pgate[i] = 0u;
      }
      pending = false;
    } else {
      for (pht_ctx *c : ctxs) {
        memcpy(c->h_params.get(), pb.data(), pb.size());
        if (c->grp) {
          if (group_sweep(c, k0, k1, (uint32_t)iter, zexp)) return -1;
        } else if (ctx_enqueue(c, k0, k1, (uint32_t)iter, zexp, false, timed)) {
          return -1;
        }
      }
    }
    if (pipe && iter + 1 < it) {
      for (size_t i = 0; i < ctxs.size(); i++) {
        pht_ctx *c = ctxs[i];
        if (++c->gate_seq == 0u) c->gate_seq = 1u;
        /* (recorded first: a failed enqueue may have left the gate kernel in
         * the stream, and unwind releases it) */
        pgate[i] = c->gate_seq;
        if (ctx_enqueue(c, k0, k1, (uint32_t)(iter + 1), zexp, false, want_time(iter + 1), pgate[i])) {
          unwind();
          return -1;
        }
      }
      pending = true;
    }
    std::fill(tot.begin(), tot.end(), 0LL);
    bool wrapped = false;
    bool any_t = false;
    double ksum = 0.0;
    for (pht_ctx *c : ctxs) {
      if (!c->grp && ctx_wait(c)) {
        unwind();
        return -1;
      }
      if (c->last_ms >= 0.f) {
        ksum += c->last_ms;
        any_t = true;
      }
      for (int k = 0; k < sl; k++) wrapped |= __builtin_add_overflow(tot[k], (long long)c->h_stats.get()[k], &tot[k]);
    }
    if (reduce && reduce(tot.data(), sl, reduce_user) != 0) {
      set_err("statistics all-reduce callback failed at sweep %d", iter);
      unwind();
      return -1;
    }
#ifndef PHT_STAMPS /* diagnostic builds carry cycle stamps in the extra words */
    const long long *xw = tot.data() + 2 * n + n * n;
    if (expect >= 0 && xw[kXObs] != expect) {
      set_err("sweep %d sampled %lld observations, expected %lld: the statistics are incomplete or summed twice",
              iter, xw[kXObs], expect);
      unwind();
      return -1;
    }
    for (int k = 0; k < n; k++) wrapped |= tot[k] < 0;
    if (wrapped || xw[kXOverflow] != 0) {
      set_err("sweep %d: the fixed-point z sums overflowed int64 (zexp = %d leaves 2^%d time units; censored paths "
              "ran far past the observed times): pass a smaller zexp",
              iter, zexp, 63 - zexp);
      unwind();
      return -1;
    }
    /* observations that hit a cap (ARMS iterations, path length, MHRS
     * attempts) or a numerical guard contribute their last attempt, where
     * the reference would keep looping (DESIGN.md §3 Caps) */
    const long long fl = xw[kXFlagged];
    if (fl > 0) {
      if (!first_flagged) first_flagged = iter;
      flagged += fl;
    }
    /* UNIF observations beyond the table or the lam cap carry a path that is
     * not a draw of the target law (pht_unif.h): an error, not a warning.
     * Only sweeps that ran the UNIF kernels: other samplers' diagnostic
     * builds (PHT_ECS_DIAG, PHT_DCS_DIAG) count their own things in word 6 */
    if (bm == kMethodUNIF && xw[kXUnifCap] > 0) {
      set_err("sweep %d: %lld UNIF observations need more than %d uniformisation steps or mu*y > %g (the largest "
              "exit rate times the largest observation); their paths would be wrong: rescale the data",
              iter, xw[kXUnifCap], kUnifMaxK, kUnifMaxLam);
      unwind();
      return -1;
    }
#endif
    if (any_t) {
      kms += ksum;
      ktimed++;
    }
    for (int k = 0; k < n; k++) z[k] = ldexp((double)tot[k], -zexp);
    G.update(R, iter, z.data(), tot.data() + 2 * n);
  }
  if (ktimed > 0) kms = kms / (double)ktimed * (double)(it - 1);
  for (pht_ctx *c : ctxs) c->flagged = flagged;
  if (flagged)
    warn("\nWARNING: %lld observation-sweeps hit a sampler cap or numerical guard (first in iteration %d); "
         "each contributed its last attempt to the sufficient statistics\n",
         flagged, first_flagged + 1);
  if (kernel_ms_total) *kernel_ms_total = kms;
  return 0;
}
/* the two streams a loop is driven by: R's (or its stand-in), a chain's own */
template int pht::host::gibbs_run<RHost>(RHost &, int, int, int, int, const double *, const double *, const int *,
                                         const double *, int, const double *, double *, std::vector<pht_ctx *> &,
                                         uint32_t, uint32_t, int, pht_reduce_fn, void *, double *);
template int pht::host::gibbs_run<OwnRng>(OwnRng &, int, int, int, int, const double *, const double *, const int *,
                                          const double *, int, const double *, double *, std::vector<pht_ctx *> &,
                                          uint32_t, uint32_t, int, pht_reduce_fn, void *, double *);

/*
 * Multi-process entry (one process per GPU): this process owns observations
 * [obs0, obs0 + l) of a data set of l_total observations (zexp must be the
 * same on every rank: pht_zexp over all observations); `reduce` sums the
 * statistics block across ranks (e.g. an RCCL all-reduce).  The R-stream
 * (pht_set_seed) must be seeded identically on all ranks; every rank then
 * draws identical Gamma updates and the chain is the single-process chain.
 */
extern "C" int pht_gibbs_run(pht_ctx *c, int it, int method, int m, const double *nu, const double *zeta,
                             const int *T, const double *C, int zexp, int silent, const double *start, double *res,
                             pht_reduce_fn reduce, void *reduce_user, double *kernel_ms_total) {
  if (!c) {
    set_err("pht_gibbs_run: null context");
    return -1;
  }
  if (reduce && c->comm) {
    /* the block would be summed twice: by RCCL on the stream, then here */
    set_err("pht_gibbs_run: a reduce callback was given for a context with an RCCL communicator attached");
    return -1;
  }
  RHost &R = rhost();
  R.begin();
  const uint32_t k0 = (uint32_t)(R.u() * 4294967296.0);
  const uint32_t k1 = (uint32_t)(R.u() * 4294967296.0);
  std::vector<pht_ctx *> ctxs{c};
  int rc = gibbs_run(R, it, method, c->n, m, nu, zeta, T, C, silent, start, res, ctxs, k0, k1, zexp, reduce,
                     reduce_user, kernel_ms_total);
  R.end();
  return rc;
}
extern "C" int pht_theta_to_S(int n, int m, const int *T, const double *C, const double *theta, double *S,
                              double *s) {
  if (n < 1 || n > kMaxN || m < 1 || !T || !C || !theta || !S || !s) {
    set_err("pht_theta_to_S: invalid argument");
    return -1;
  }
  const int n1 = n + 1;
  ParamLists L;
  if (L.build(n, m, T, C)) {
    char why[160];
    L.describe(why, sizeof why);
    set_err("pht_theta_to_S: %s", why);
    return -1;
  }
  std::vector<double> TT((size_t)n1 * n1, 0.0);
  for (int k = 0; k < m; k++)
    for (const Ent &e : L.TTl[k]) TT[e.i + e.j * n1] = tt_cell(theta[k], e.c);
  /* the diagonal as GibbsState::update leaves it for every drawn row */
  for (int i = 0; i < n; i++) TT[i + i * n1] = tt_diag(n1, T, TT.data(), i, true);
  tt_split(n, TT.data(), S, s);
  return 0;
}
