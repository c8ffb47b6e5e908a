/*
 * phasetype_amd.h — C ABI of the MI355X-native PhaseType hot path
 * (libPhaseType.so, built by phasetype_amd/build.py).
 *
 * 1. Drop-in boundary (what R binds).  The reference registers exactly one
 *    native routine, for `.C`:
 *      src/PHT_MCMC_Aslett.h:1-3    void LJMA_Gibbs(int*, int*, int*, int*, int*, double*, double*,
 *                                                   int*, double*, double*, int*, int*, double*, int*, double*)
 *      src/Registrations.c:6-20     R_init_PhaseType: R_registerRoutines(.C, 15 typed args),
 *                                   R_useDynamicSymbols(FALSE), R_forceSymbols(TRUE)
 *      NAMESPACE:2                  useDynLib(PhaseType, .registration = TRUE)
 *    Callers: R/phtMCMC.R:83, R/phtMCMC2.R:73.  Same names, same argument
 *    meaning, same output layout (res[iter + i*it]); see INTEGRATION.md.
 *
 * 2. Sweep-level ABI (the seam the reference's LJMA_MHsample_{Bladt,
 *    Aslett2,Hobolth2} occupy, src/PHT_MCMC_Aslett.c:325-333): one Gibbs
 *    step 1 over a shard of observations on one GPU, returning the int64
 *    sufficient-statistics block
 *      [zq n][B n][N n*n][16 counters]   (pht_stats_len(n) entries)
 *    zq = z in fixed point, z_k = zq_k * 2^-zexp; N[i + j n] = i->j
 *    transitions, diagonal = absorb-from counts (reference convention).
 *
 * Errors: functions returning int return 0 on success and non-zero on
 * failure with a message in pht_last_error().  There is no CPU fallback:
 * without a HIP device, pht_ctx_create and LJMA_Gibbs fail loudly.
 */
#ifndef PHASETYPE_AMD_H
#define PHASETYPE_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- drop-in boundary ------------------------------------------------ */
void LJMA_Gibbs(int *it, int *mhit, int *method, int *n, int *m, double *nu, double *zeta, int *T, double *C,
                double *y, int *l, int *censored, double *start, int *silent, double *res);
void R_init_PhaseType(void *dll_info);

/* ---- host services ----------------------------------------------------- */
const char *pht_last_error(void);
int pht_device_count(void);
/* Bind an LP64 LAPACK (dgeevx_/dgetrf_/dgetri_ with symbol prefix); inside R
 * the process's own LAPACK is found automatically. */
int pht_bind_lapack(const char *path, const char *prefix);
/* Standalone R-compatible random stream (ignored inside R): set.seed(seed). */
void pht_set_seed(uint32_t seed);
double pht_unif_rand(void);
double pht_rgamma(double shape, double scale);
int pht_in_R(void);
void pht_set_verbose(int v);
int pht_zexp(const double *y, long l);
int pht_params_bytes(int n);
int pht_stats_len(int n);
int pht_build_params(int n, const double *S, const double *s, int method, unsigned char *out, int out_bytes);

/* ---- sweep-level ABI ----------------------------------------------------- */
typedef struct pht_ctx pht_ctx;
pht_ctx *pht_ctx_create(int device, int n, int method, int mhit);
void pht_ctx_destroy(pht_ctx *c);
int pht_ctx_set_obs(pht_ctx *c, const double *y, const int *censored, long count, long obs0);
int pht_ctx_sweep(pht_ctx *c, const double *S, const double *s, uint32_t k0, uint32_t k1, uint32_t sweep,
                  int zexp, long long *stats_out);
int pht_ctx_sweep_debug(pht_ctx *c, const double *S, const double *s, uint32_t k0, uint32_t k1, uint32_t sweep,
                        int zexp, long long *stats_out, int *B, int *pre, int *flags, uint32_t *ndraw,
                        long long *zq, int *N);
/* Device time of the last sweep's kernels (HIP events); -1 when that sweep
 * was not timed (pht_gibbs_run times one sweep in PHT_KTIME_EVERY). */
float pht_ctx_last_kernel_ms(pht_ctx *c);
/* Observation-sweeps flagged in the last pht_gibbs_run / pht_gibbs_run_chains
 * on this context (node-wide, after the reduce): a cap (ARMS iterations, path
 * length, MHRS attempts) or a numerical guard fired, and the observation
 * contributed its last attempt.  No reference counterpart (its loops are
 * unbounded); a warning is also printed once per run. */
long long pht_ctx_flagged_obs(pht_ctx *c);
/* Observations over ALL shards of a multi-process run (this context's shard
 * included).  pht_gibbs_run checks every sweep that the node-wide statistics
 * account for exactly this many observations, and fails the run otherwise
 * (single process: the check uses the context's own count, always on).  No
 * reference counterpart (the reference has one process and no such failure
 * mode, src/PHT_MCMC_Aslett.c:325-337). */
int pht_ctx_set_global_count(pht_ctx *c, long long total);

/* Gibbs loop over one shard; reduce(stats, len, user) must sum the int64
 * block across all shards (return 0 on success), or NULL (single process, or
 * an RCCL communicator attached: passing both is an error, the block would be
 * summed twice).  Every sweep is checked: the node-wide processed count must
 * equal the observations (see pht_ctx_set_global_count), and the fixed-point
 * z sums must not overflow int64; either failure ends the run with an error.
 * kernel_ms_total: the sweeps' device time, measured by HIP events on one
 * sweep in PHT_KTIME_EVERY (default 4; the events cost the GPU ~9 us of idle
 * time per timed sweep) and scaled to all it - 1 sweeps from their mean. */
typedef int (*pht_reduce_fn)(long long *stats, int len, void *user);
int pht_gibbs_run(pht_ctx *c, int it, int method, int m, const double *nu, const double *zeta, const int *T,
                  const double *C, int zexp, int silent, const double *start, double *res, pht_reduce_fn reduce,
                  void *reduce_user, double *kernel_ms_total);

/* Multi-process runs without a host callback: every sweep's statistics
 * block on this context is summed over `nranks` processes by an RCCL
 * all-reduce (uint64, in place) on the context's stream, before its copy to
 * the host; pht_gibbs_run then takes reduce = NULL.  One rank calls
 * pht_rccl_unique_id and broadcasts the 128 bytes; every rank first calls
 * pht_ctx_rccl_prepare (all LOCAL preconditions: RCCL loadable, no
 * communicator yet, device, staging buffer of max_len words), the ranks agree
 * on its verdict, and only then every rank attaches with the same id (the
 * collective ncclCommInitRank).  RCCL is loaded at run time (librccl.so.1).
 * No reference counterpart: the reference is single-process
 * (src/PHT_MCMC_Aslett.c:325-337). */
int pht_rccl_unique_id(unsigned char *id128);
int pht_ctx_rccl_prepare(pht_ctx *c, int max_len);
int pht_ctx_attach_rccl(pht_ctx *c, const unsigned char *id128, int nranks, int rank);
/* In-place sum of buf[len] (host int64, len <= the prepared max_len) over the
 * attached communicator, on the context's stream: the all-reduce a sweep runs
 * on its statistics block, exposed so the caller can check it against its own
 * collective.  Once attached, a rank always enters the collective. */
int pht_ctx_rccl_allreduce(pht_ctx *c, long long *buf, int len);

/* Device-resident Gibbs chain (opt-in, NON-PARITY):
 * the conjugate Gamma update (src/PHT_MCMC_Aslett.c:340-397) and the next
 * sweep's parameter block (:279-297) run on the device between sweeps
 * (phasetype_amd/csrc/pht_resident.hip), so the host enqueues every sweep
 * and waits once.  Gamma draws come from a counter-based sampler
 * (include/pht_gamma.h), not R's rgamma: the chain is deterministic under
 * set.seed but not the host loop's chain.  Any method matching the context's
 * (for ECS/DCS the update also builds the eigensystem, include/pht_eigen.h,
 * instead of LAPACK: a complex spectrum stops the run with an error, where the
 * host path warns and uses the real parts as the reference does, and so does a
 * defective or nearly defective S, whose eigenvectors do not reproduce it:
 * PHT_EIG_RESID_TOL); an attached RCCL
 * communicator sums every sweep's statistics on the stream (every rank must
 * use the same R-stream seed).  Arguments and res layout as pht_gibbs_run;
 * kernel_ms_total = device time of all sweeps. */
int pht_gibbs_run_resident(pht_ctx *c, int it, int method, int m, const double *nu, const double *zeta, const int *T,
                           const double *C, int zexp, const double *start, double *res, double *kernel_ms_total);

/* Independent chains at once (no reference counterpart —
 * the reference runs one chain per LJMA_Gibbs call, src/PHT_MCMC_Aslett.c:104):
 * chain c on ctxs[c] (one context each, same n/method/mhit, observations set),
 * its own host thread and R-compatible stream seeded by seeds[c]; chain c
 * equals pht_gibbs_run after pht_set_seed(seeds[c]).  res: nchains blocks of
 * it*m (pht_gibbs_run's layout); start: exactly nchains*m values (chain c
 * reads start[c*m .. c*m+m-1]) or start[0] < 0 — the length is not checked
 * here, so a caller holding one m-vector must repeat it per chain (the
 * Python mirror phasetype_amd.gibbs_chains broadcasts and validates it).
 * Standalone builds only (fails inside R), and not on contexts with an RCCL
 * communicator attached. */
int pht_gibbs_run_chains(pht_ctx **ctxs, int nchains, const uint32_t *seeds, int it, int method, int m,
                         const double *nu, const double *zeta, const int *T, const double *C, int zexp,
                         const double *start, double *res, double *kernel_ms_max);

/* ---- log-likelihood of posterior draws -------------------------------------
 * No reference counterpart (the reference returns the draws only).  The
 * observed-data log-likelihood of draw theta -> (S, s), pi = e_1:
 *   sum over exact y of log f(y) + sum over censored y of log Fbar(y),
 * evaluated on the GPU from the draw's eigensystem over the context's resident
 * observations; arithmetic and layouts are specified in include/pht_loglik.h.
 * This (default) evaluator is SPECTRAL: a draw whose spectrum is complex or
 * defective (dgeevx info, a non-zero imaginary part, a non-finite coefficient)
 * gets a non-zero flag word, is never evaluated, and reads NaN.  Such draws
 * are served by the second evaluator, by uniformisation (pht_ctx_loglik_unif
 * below; include/pht_loglik_unif.h).
 *
 * pht_loglik_build: host only (no GPU), one draw's block of pht_loglik_bytes(n)
 *   bytes; returns 0, the positive flag word of an unusable draw, < 0 on error.
 * pht_theta_to_S: one row of the chain -> (S, s) (column-major n x n, n), with
 *   the T / C maps of pht_gibbs_run and the diagonal order of its update.
 * pht_ctx_loglik: ndraws blocks, `batch` (1..64) per launch, on the context's
 *   stream; any method's context; fails (no launch) without observations.
 *   totals: 4 int64 words per draw [H, F, nbad, nobs]: the draw's
 *   log-likelihood is H + F 2^-32 over its nobs good observations (exact
 *   integer sums: independent of batch, grid and shard, and summed across
 *   ranks like the statistics block); nbad observations had a non-positive or
 *   non-finite density and are left out.  All four stay 0 for a flagged draw.
 *   pointwise: NULL, or ndraws * count values l[d * count + i] in the caller's
 *   observation order (NaN where bad or flagged).  accumulate != 0: the
 *   per-observation WAIC state (pht_waic_t) takes every finite l, in draw order.
 *   pht_ctx_last_kernel_ms then gives the device time of the call's launches.
 * pht_ctx_loglik_reset zeroes that state; pht_ctx_loglik_state copies it out
 *   in the caller's observation order (count values each). */
int pht_loglik_bytes(int n);
int pht_loglik_build(int n, const double *S, const double *s, unsigned char *out, int out_bytes);
int pht_theta_to_S(int n, int m, const int *T, const double *C, const double *theta, double *S, double *s);
int pht_ctx_loglik(pht_ctx *c, int ndraws, const unsigned char *blocks, int batch, long long *totals,
                   double *pointwise, int accumulate);
int pht_ctx_loglik_reset(pht_ctx *c);
int pht_ctx_loglik_state(pht_ctx *c, double *ref, double *S1, double *S2, double *m, double *r, int *cnt);

/* The same log-likelihood by uniformisation (include/pht_loglik_unif.h): sums
 * of non-negative terms straight from (S, s), no eigensystem and no LAPACK, so
 * it serves complex and defective spectra and does not lose cond(Q) ulps.
 * Limits: pi = e_1; the table cap of 2047 rows, roughly mu y <= 1500 with
 * mu = max_i -S_ii; a Poisson-weighted sum below 2^-900.  Beyond either the
 * observation is bad for that draw (counted in nbad), as in pht_ctx_loglik.
 *
 * pht_ctx_loglik_unif: ndraws draws, S the column-major n x n generators one
 *   after another, s the n-vectors; batch, totals, pointwise and accumulate as
 *   in pht_ctx_loglik, and the WAIC state is the same one: calls of either
 *   kind with accumulate continue it in call order.  flags_out: NULL, or
 *   ndraws flag words (0 = evaluated; PHT_LL_F_NONFINITE 4: a non-finite entry;
 *   PHT_LL_F_MU 8: mu not positive and finite); a flagged draw is skipped like
 *   a flagged block.  The tables live in a buffer of their own: a UNIF
 *   (method 8) context's chain is not affected.
 * pht_ctx_loglik_unif_K: the last table row K the context would use for a
 *   draw with this mu (from its largest observation), < 0 on error. */
int pht_ctx_loglik_unif(pht_ctx *c, int ndraws, const double *S, const double *s, int batch, long long *totals,
                        double *pointwise, int accumulate, int *flags_out);
int pht_ctx_loglik_unif_K(pht_ctx *c, double mu);

/* Expected sufficient statistics given the observations (the E-step;
 * include/pht_estep.h is the whole definition): per draw (S, s), summed over
 * the context's observations, Z_i = E[time in state i | y], N_ij =
 * E[transitions i -> j | y] and E_i = E[exits from i | y] on [0, y], and A_i =
 * the expected number of censored observations in state i at y, by the same
 * uniformisation as pht_ctx_loglik_unif (its limits apply: pi = e_1, the table
 * cap, bad observations counted in nbad and left out).  No reference
 * counterpart.  The observations enter through int64 histograms only: per
 * draw pht_estep_words() = 8192 words [class][k][G, T] (class 0 exact, 1
 * censored; 2048 rows each), exact integer sums that do not depend on batch,
 * grid or shard and add across shards and ranks (the caller's reduce, or
 * pht_ctx_rccl_allreduce) PROVIDED every shard uses the same yscale, a power
 * of two >= every observation of every shard.  Limit: at most 2^22
 * observations in all shards together (the context's count, or its
 * pht_ctx_set_global_count); beyond it the call fails.
 *
 * pht_ctx_estep: ndraws draws as in pht_ctx_loglik_unif, `batch` (1..64) per
 *   launch.  yscale: <= 0 for the default, pht_estep_yscale(largest
 *   observation of this context).  totals: ndraws * 4 int64 [H, F, nbad, nobs],
 *   bit for bit pht_ctx_loglik_unif's.  words: NULL, or ndraws * 8192 int64.
 *   Z (ndraws * n), N (ndraws * n * n, N[i + j n] from i to j, diagonal 0),
 *   E, A (ndraws * n each): all four, or all NULL for the histograms alone (callers
 *   that reduce across ranks first, then pht_estep_contract).  A flagged draw
 *   (flags_out as in pht_ctx_loglik_unif) has zero words and NaN statistics.
 *   The buffers are the context's own: its chain is not affected.
 * pht_estep_contract: host only (no GPU), one draw's Z, N, E, A from its
 *   (summed) words, rows 0..K (K = 2047 for words of pht_ctx_estep); bit for
 *   bit what the device computes.  Returns the draw's flag word, < 0 on error.
 * pht_ctx_estep_grid_cap: the most blocks of the histogram kernel (0: the
 *   default, one a CU); the results do not depend on it.
 * pht_ctx_estep_ms: device time of the last call, the histograms (with the
 *   tables) and the contraction. */
int pht_estep_words(void);
double pht_estep_yscale(double ymax);
int pht_ctx_estep(pht_ctx *c, int ndraws, const double *S, const double *s, int batch, double yscale,
                  long long *totals, long long *words, double *Z, double *N, double *E, double *A, int *flags_out);
int pht_estep_contract(int n, const double *S, const double *s, const long long *words, int K, double yscale,
                       double *Z, double *N, double *E, double *A);
int pht_ctx_estep_grid_cap(pht_ctx *c, int cap);
int pht_ctx_estep_ms(pht_ctx *c, float *hist_ms, float *contract_ms);

/* Quantiles and residual-life quantiles (include/pht_quantile.h is the whole
 * definition): per draw (S, s) with pi = e_1 and per probability p, the t >= t0
 * with P(T <= t | T > t0) = p, by a safeguarded Newton iteration on the log
 * survival function of pht_ctx_loglik_unif's evaluator.  No reference
 * counterpart, and no observations are needed on the context.
 *
 * pht_ctx_quantile: ndraws draws as in pht_ctx_loglik_unif, `batch` (1..64) per
 *   launch; np probabilities in any order, duplicates allowed; t0 >= 0 the
 *   conditioning time (0: the plain quantile function); tmax > 0 the horizon
 *   (+inf: as far as the table cap allows, 1400 / max_i -S_ii).  Outputs, each
 *   ndraws * np in the caller's order of probs (all but t_out may be NULL):
 *   t_out the quantile (t - t0 for t0 > 0, a residual life), lo_out and hi_out
 *   the final bracket (absolute times), nev_out the evaluations of the root,
 *   flags_out the PHT_Q_F_* bits; draw_flags_out (ndraws) as in
 *   pht_ctx_loglik_unif.  p = 0 gives 0 and p = 1 +inf without a flag; a root
 *   beyond the horizon +inf with PHT_Q_F_BEYOND; every other flag NaN.  The
 *   buffers are the context's own: its chain and its WAIC state are not
 *   affected.
 * pht_ctx_quantile_ms: device time of the last call, the table kernel and the
 *   searches.
 * pht_quantile_host: host only (no GPU), one draw; bit for bit what the device
 *   computes.  Returns the draw's flag word, < 0 on error. */
int pht_ctx_quantile(pht_ctx *c, int ndraws, const double *S, const double *s, int np, const double *probs,
                     double t0, double tmax, int batch, double *t_out, double *lo_out, double *hi_out, int *nev_out,
                     unsigned *flags_out, int *draw_flags_out);
int pht_ctx_quantile_ms(pht_ctx *c, float *table_ms, float *search_ms);
int pht_quantile_host(int n, const double *S, const double *s, int np, const double *probs, double t0, double tmax,
                      double *t_out, double *lo_out, double *hi_out, int *nev_out, unsigned *flags_out);

/* Age-replacement policies (include/pht_replace.h is the whole definition): a
 * unit is replaced at failure (cost cf) or at age tau (cost cp < cf),
 * whichever comes first; per draw (S, s) with pi = e_1 the long-run cost rate
 * g(tau) = (cp + (cf - cp) F(tau)) / M(tau), M the restricted mean life, on a
 * grid of ages, and per cost pair the age that minimises it (the grid's argmin
 * refined by a 64-way multisection on the sign of g').  No reference
 * counterpart, and no observations are needed on the context.
 *
 * pht_ctx_replace: ndraws draws as in pht_ctx_loglik_unif, `batch` (1..64) per
 *   launch; G ages (1..1024), finite, positive, strictly increasing; P cost
 *   pairs (1..16).  Policy outputs, each ndraws * P (all but t_out and g_out
 *   may be NULL): t_out the optimal age (+inf with PHT_RP_F_NEVER when running
 *   to failure costs no more), g_out its cost rate, lo_out and hi_out the final
 *   bracket, j_out the grid's argmin, nev_out the points evaluated, flags_out
 *   the PHT_RP_F_* bits.  Per draw (may be NULL): m_out the mean life,
 *   draw_flags_out as in pht_ctx_loglik_unif with PHT_CD_F_TRAP.  The curve,
 *   each ndraws * G (may be NULL): lS_out = log Fbar, lf_out = log f, M_out and
 *   aflags_out the PHT_RP_A_* bits (a flagged age is NaN).  The buffers are the
 *   context's own: its chain, its WAIC state and the other analyses are not
 *   affected.
 * pht_ctx_replace_ms: device time of the last call, the tables with the curve
 *   and the policies.
 * pht_replace_host: host only (no GPU), one draw; bit for bit what the device
 *   computes.  Returns the draw's flag word, < 0 on error. */
int pht_ctx_replace(pht_ctx *c, int ndraws, const double *S, const double *s, int G, const double *ages, int P,
                    const double *cp, const double *cf, int batch, double *t_out, double *g_out, double *lo_out,
                    double *hi_out, int *j_out, int *nev_out, unsigned *flags_out, double *m_out,
                    int *draw_flags_out, double *lS_out, double *lf_out, double *M_out, unsigned *aflags_out);
int pht_ctx_replace_ms(pht_ctx *c, float *curve_ms, float *policy_ms);
int pht_replace_host(int n, const double *S, const double *s, int G, const double *ages, int P, const double *cp,
                     const double *cf, double *t_out, double *g_out, double *lo_out, double *hi_out, int *j_out,
                     int *nev_out, unsigned *flags_out, double *m_out, double *lS_out, double *lf_out, double *M_out,
                     unsigned *aflags_out);

/* Fleet forecasts (include/pht_forecast.h is the whole definition): for every
 * draw (S, s) with pi = e_1, every right-censored observation c_i of the
 * context (a unit still in service at age c_i) and every horizon h_j, the
 * conditional failure probability q = P(T <= c_i + h_j | T > c_i), by
 * pht_ctx_loglik_unif's evaluator at c_i and at c_i + h_j.  No reference
 * counterpart.  Limits: pi = e_1, at most 16 horizons, at most 2^22 censored
 * units per context, mu (c + h) up to roughly 1500 (beyond: the unit is bad
 * for that draw and horizon, counted and never summed).
 *
 * pht_ctx_forecast: ndraws draws as in pht_ctx_loglik_unif, `batch` (1..64)
 *   per launch; nh (1..16) horizons, each finite, >= 0, strictly increasing.
 *   words_out: int64 [ndraws][nh][4] = [M, V, nbad, nunits], M and V the sums
 *   of llrint(q 2^40) and llrint(q (1 - q) 2^40) over the units good for that
 *   draw and horizon (exact integer sums: shards and ranks add them); a
 *   flagged draw's words are zero.  qsum_out (double) and cnt_out (int64),
 *   each [ncens][nh] in the caller's order of the censored observations and
 *   started from zero by every call: the sum of q over the draws in which the
 *   unit was good, in draw order, and their number.  q_out: NULL, or
 *   [ndraws][ncens][nh], NaN where bad (tests and small fleets).
 *   draw_flags_out (ndraws, may be NULL) as in pht_ctx_loglik_unif.  Refused
 *   with a message: no censored observation on the context, more than 2^22,
 *   nh or a horizon outside the above, batch outside 1..64.  The buffers are
 *   the context's own: its chain and its WAIC state are not affected.
 * pht_ctx_forecast_units: the number of censored units of the context; with
 *   idx_out (that many), their indices in the caller's observation order.
 * pht_ctx_forecast_grid_cap: most blocks of the kernel (0: the default); the
 *   result does not depend on it.
 * pht_ctx_forecast_ms: device time of the last call, the table kernel and the
 *   evaluations.
 * pht_forecast_host: host only (no GPU), one draw over `ncens` ages; bit for
 *   bit what the device computes.  ymax_c: the largest censored observation
 *   the table is sized for (0: the largest of ages).  words_out [nh][4] is
 *   written; qsum and cnt ([ncens][nh], may be NULL) are UPDATED (one call
 *   per draw, in order); q_out ([ncens][nh], may be NULL) is written.  Returns
 *   the draw's flag word, < 0 on error. */
int pht_ctx_forecast(pht_ctx *c, int ndraws, const double *S, const double *s, int nh, const double *horizons,
                     int batch, long long *words_out, double *qsum_out, long long *cnt_out, double *q_out,
                     int *draw_flags_out);
long pht_ctx_forecast_units(pht_ctx *c, long *idx_out);
int pht_ctx_forecast_grid_cap(pht_ctx *c, int cap);
int pht_ctx_forecast_ms(pht_ctx *c, float *table_ms, float *eval_ms);
int pht_forecast_host(int n, const double *S, const double *s, long ncens, const double *ages, int nh,
                      const double *horizons, double ymax_c, long long *words_out, double *qsum, long long *cnt,
                      double *q_out);

/* Fleet condition (include/pht_condition.h is the whole definition): for every
 * draw (S, s) with pi = e_1 and every right-censored observation c_i of the
 * context (a unit still in service at age c_i), the posterior law phi of the
 * PHASE the unit is in given that it has survived to c_i, its mean residual
 * life MRL = phi . (-S)^-1 1 and, per horizon h_j, the expected number of
 * failures D = phi . r_h when every failed unit is replaced by a new one.  No
 * reference counterpart.  Limits: pi = e_1, 0 to 16 horizons with mu h up to
 * roughly 1450, at most 2^22 censored units per context, mu c up to roughly
 * 1500 (beyond: the unit is bad for that draw, counted and never summed).
 *
 * pht_ctx_condition: ndraws draws as in pht_ctx_loglik_unif, `batch` (1..64)
 *   per launch; nh (0..16) horizons as in pht_ctx_forecast.  words_out: int64
 *   [ndraws][n + nh + 3] = [Phi_0 .. Phi_{n-1}, L, Delta_0 .. Delta_{nh-1},
 *   nbad, nunits], the sums over the units good for that draw of
 *   llrint(phi_j 2^40), llrint((MRL / mscale) 2^40) and
 *   llrint((D_j / dscale_j) 2^40) (exact integer sums: shards and ranks add
 *   them); scales_out: [ndraws][1 + nh] = [mscale, dscale_j], powers of two
 *   that depend on the draw alone; both zero for a flagged draw.  phisum_out
 *   [ncens][n], mrlsum_out [ncens], dsum_out [ncens][nh] (double) and cnt_out
 *   [ncens] (int64), in the caller's order of the censored observations and
 *   started from zero by every call: the sums over the draws in which the unit
 *   was good, in draw order, and their number.  phi_out: NULL, or
 *   [ndraws][ncens][n], with mrl_out [ndraws][ncens] and d_out
 *   [ndraws][ncens][nh] (each NULL or given), NaN where bad (tests and small
 *   fleets).  draw_flags_out (ndraws, may be NULL): pht_ctx_loglik_unif's flag
 *   words and 64 (a state that cannot reach absorption), 128 (mu h_max beyond
 *   the renewal table); a flagged draw is skipped.  Refused with a message: no
 *   censored observation on the context, more than 2^22, nh or a horizon
 *   outside the above, batch outside 1..64.  The buffers are the context's
 *   own: its chain, its WAIC state and its forecast state are not affected.
 * pht_ctx_condition_grid_cap: most blocks of the unit kernel (0: the default);
 *   the result does not depend on it.
 * pht_ctx_condition_ms: device time of the last call, the table kernels and
 *   the unit kernel.
 * pht_condition_host: host only (no GPU), one draw over `ncens` ages; bit for
 *   bit what the device computes.  ymax_c: the largest censored observation
 *   the tables are sized for (0: the largest of ages).  words_out
 *   [n + nh + 3] and scales_out [1 + nh] are written; phisum, mrlsum, dsum and
 *   cnt (may be NULL) are UPDATED (one call per draw, in order); phi_out,
 *   mrl_out, d_out (may be NULL) are written.  Returns the draw's flag word,
 *   < 0 on error. */
int pht_ctx_condition(pht_ctx *c, int ndraws, const double *S, const double *s, int nh, const double *horizons,
                      int batch, long long *words_out, double *scales_out, double *phisum_out, double *mrlsum_out,
                      double *dsum_out, long long *cnt_out, double *phi_out, double *mrl_out, double *d_out,
                      int *draw_flags_out);
int pht_ctx_condition_grid_cap(pht_ctx *c, int cap);
int pht_ctx_condition_ms(pht_ctx *c, float *table_ms, float *unit_ms);
int pht_condition_host(int n, const double *S, const double *s, long ncens, const double *ages, int nh,
                       const double *horizons, double ymax_c, long long *words_out, double *scales_out,
                       double *phisum, double *mrlsum, double *dsum, long long *cnt, double *phi_out, double *mrl_out,
                       double *d_out);

/* Fleet spares (include/pht_spares.h is the whole definition): for every draw
 * (S, s) with pi = e_1, every right-censored observation c_i of the context (a
 * unit still in service at age c_i) and every horizon h_j, the mean D and the
 * VARIANCE var of the number of failures within h_j when every failed unit is
 * replaced by a new one (D is pht_ctx_condition's, bit for bit; var = Q + D -
 * D^2 with Q = phi . q_h the second factorial moment).  The draws' moment
 * vectors are built on the device.  No reference counterpart.  Limits: the
 * condition's, and 1 to 16 horizons.
 *
 * pht_ctx_spares: ndraws draws as in pht_ctx_condition, `batch` (1..64) per
 *   launch; nh (1..16) horizons.  words_out: int64 [ndraws][2 nh + 2] =
 *   [Delta_0 .. Delta_{nh-1}, V_0 .. V_{nh-1}, nbad, nunits], the sums over the
 *   units good for that draw of llrint((D_j / dscale_j) 2^40) and
 *   llrint((var_j / vscale_j) 2^40) (exact integer sums: shards and ranks add
 *   them; the units are independent given the draw, so V is the fleet's
 *   variance within the draw); scales_out: [ndraws][2 nh] = [dscale_j,
 *   vscale_j], powers of two that depend on the draw alone; both zero for a
 *   flagged draw.  dsum_out, vsum_out, d2sum_out [ncens][nh] (double: the sums
 *   of D, var and D D) and cnt_out [ncens] (int64), in the caller's order of
 *   the censored observations and started from zero by every call: the sums
 *   over the draws in which the unit was good, in draw order, and their
 *   number.  d_out: NULL, or [ndraws][ncens][nh] with var_out of the same
 *   shape, NaN where bad (tests and small fleets).  draw_flags_out (ndraws,
 *   may be NULL): pht_ctx_condition's flag words for the same input; a flagged
 *   draw is skipped.  Refused with a message: no censored observation on the
 *   context, more than 2^22, nh or a horizon outside the above, batch outside
 *   1..64.  The buffers are the context's own: its chain, its WAIC state, its
 *   forecast state and its condition buffers are not affected.
 * pht_ctx_spares_grid_cap: most blocks of the unit kernel (0: the default);
 *   the result does not depend on it.
 * pht_ctx_spares_ms: device time of the last call, the vectors kernel with
 *   the table kernels, and the unit kernel.
 * pht_spares_host: host only (no GPU), one draw over `ncens` ages; bit for
 *   bit what the device computes.  ymax_c: the largest censored observation
 *   the tables are sized for (0: the largest of ages).  words_out [2 nh + 2]
 *   and scales_out [2 nh] are written; dsum, vsum, d2sum and cnt (may be NULL)
 *   are UPDATED (one call per draw, in order); d_out, var_out (may be NULL)
 *   are written.  Returns the draw's flag word, < 0 on error. */
int pht_ctx_spares(pht_ctx *c, int ndraws, const double *S, const double *s, int nh, const double *horizons,
                   int batch, long long *words_out, double *scales_out, double *dsum_out, double *vsum_out,
                   double *d2sum_out, long long *cnt_out, double *d_out, double *var_out, int *draw_flags_out);
int pht_ctx_spares_grid_cap(pht_ctx *c, int cap);
int pht_ctx_spares_ms(pht_ctx *c, float *vector_ms, float *unit_ms);
int pht_spares_host(int n, const double *S, const double *s, long ncens, const double *ages, int nh,
                    const double *horizons, double ymax_c, long long *words_out, double *scales_out, double *dsum,
                    double *vsum, double *d2sum, long long *cnt, double *d_out, double *var_out);

/* PSIS-LOO cross-validation with Pareto-k diagnostics (include/pht_psis.h is
 * the whole definition): per observation, from l[d, i] of every usable draw
 * at once, elpd_loo_i, the Pareto shape khat_i of the importance ratios' tail
 * and lppd_i.  The pointwise matrix stays on the device: ndraws * count * 8
 * bytes (plus a transposed chunk of at most 256 MB and 28 bytes per
 * observation), which must fit the device's free memory with 512 MB to spare;
 * there is no chunking over observations: thin the chain instead.  Limits:
 * 1 <= ndraws <= 16384; smoothing needs at least 25 usable draws.
 *
 * pht_ctx_loo_begin: allocates the matrix for ndraws rows and marks every row
 *   unusable; fails (message in pht_last_error) when it does not fit, without
 *   observations, or with ndraws out of range.  A new pht_ctx_set_obs drops it.
 * pht_ctx_loo_fill / pht_ctx_loo_fill_unif: rows [row0, row0 + nd) from nd
 *   draws by the spectral / uniformisation evaluator, arguments and totals as
 *   in pht_ctx_loglik / pht_ctx_loglik_unif (so the trace comes with it); no
 *   host copy of the rows; the WAIC state is not touched.  A row is usable
 *   when its draw's flag word is 0.  Any row order, any split, any batch.
 * pht_ctx_loo: count values each, in the caller's observation order; flags:
 *   1 an l of a usable draw is NaN (outputs NaN), 2 fewer than 25 usable
 *   draws, 4 constant tail, 8 no finite fit (2, 4, 8: khat = +inf, elpd by
 *   plain importance sampling).  ndraws_used: NULL or the usable rows.
 *   pht_ctx_last_kernel_ms then gives the device time of its kernels.
 * pht_ctx_loo_end frees the matrix. */
int pht_ctx_loo_begin(pht_ctx *c, int ndraws);
int pht_ctx_loo_fill(pht_ctx *c, int row0, int nd, const unsigned char *blocks, int batch, long long *totals);
int pht_ctx_loo_fill_unif(pht_ctx *c, int row0, int nd, const double *S, const double *s, int batch,
                          long long *totals, int *flags_out);
int pht_ctx_loo(pht_ctx *c, double *elpd, double *khat, double *lppd, int *flags, int *ndraws_used);
int pht_ctx_loo_end(pht_ctx *c);

/* Posterior-predictive replicates (include/pht_predict.h): for each draw
 * (S, s), nrep absorption times of PH(e_1, S) simulated forward on the GPU, and
 * their exact integer reductions.  Limits: pi = e_1; a recorded time below
 * 2^20; at most 2^22 replicates per draw and call (more: further calls with
 * rep0 moved on; the words add); at most 1024 edges.
 *
 * pht_pred_words: the int64 words per draw (8):
 *   [Hy, Fy, Hq, Fq, ndone, nbad, nsurv, njump]: sum y = Hy + Fy 2^-32 and
 *   sum y^2 = Hq + Fq 2^-32 over the ndone recorded replicates, nsurv of them
 *   stopped at the horizon (recorded as y = horizon), njump their jumps; nbad
 *   replicates exceeded max_jumps or gave y >= 2^20 and are left out.
 * pht_pred_table_words(n): the doubles of one draw's table, n + n n.
 * pht_pred_build: host only (no GPU), one draw's table [scale n][cum n x n];
 *   returns 0 or the positive flag word of an unusable draw (PHT_LL_F_NONFINITE
 *   4: a non-finite entry; PHT_LL_F_MU 8: a diagonal not negative and finite;
 *   16: a negative rate; 32: absorption not certain from state 1; the table is
 *   then zero), < 0 on error.
 * pht_ctx_predict: nd draws (S, s as in pht_ctx_loglik_unif), `batch` (1..64)
 *   per launch, on the context's stream; any method's context, no observations
 *   needed; its buffers are its own, so the context's chain is not affected.
 *   Replicate r of draw d draws from the Philox stream (k0, k1; obs rep0 + r,
 *   a tag no sampler uses, sweep draw0 + d): a replicate's value depends on
 *   its numbers alone, never on nrep, batch or the grid.  horizon: +inf, or
 *   the time at which a path is stopped.  max_jumps: 1..2^20.  edges: ne
 *   strictly increasing finite values (ne = 0: none).
 *   words_out nd x 8; counts_out nd x (ne + 1), bin = the number of edges <= y;
 *   ymin_out / ymax_out nd (+inf / -inf where ndone = 0); all exact, so
 *   replicate ranges, batches and ranks combine by sum, min and max.
 *   y_out / njump_out: both NULL, or nd x nrep each (pointwise mode; NaN for a
 *   bad replicate and for a flagged draw).  flags_out: NULL or nd flag words as
 *   pht_pred_build returns; a flagged draw is skipped, its words stay 0.
 *   pht_ctx_last_kernel_ms then gives the device time of the call's launches. */
int pht_pred_words(void);
int pht_pred_table_words(int n);
int pht_pred_build(int n, const double *S, const double *s, double *tab, int tab_words);
int pht_ctx_predict(pht_ctx *c, int nd, const double *S, const double *s, int nrep, long long rep0, unsigned draw0,
                    unsigned k0, unsigned k1, double horizon, int max_jumps, int ne, const double *edges, int batch,
                    long long *words_out, long long *counts_out, double *ymin_out, double *ymax_out, double *y_out,
                    int *njump_out, int *flags_out);

#ifdef __cplusplus
}
#endif
#endif
