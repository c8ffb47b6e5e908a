/*
 * host_internal.h — what the units of the host runtime share: error
 * reporting, the R binding, the device context (pht_ctx), the chains group
 * and the internal functions one unit calls in another.  Nothing here is part
 * of the C ABI (include/phasetype_amd.h): it all has hidden visibility.
 *
 *   host_r.cpp         error text, R runtime and stream, LJMA_Gibbs, R_init_PhaseType
 *   host_params.cpp    LAPACK binding, eigensystem, the packed parameter block
 *   host_ctx.cpp       the context: create/destroy/set_obs, the sweep pipeline
 *   host_chains.cpp    ChainGroup, pht_gibbs_run_chains
 *   host_rccl.cpp      RCCL binding and its entry points
 *   host_gibbs.cpp     Gibbs bookkeeping and loop, pht_gibbs_run, pht_theta_to_S
 *   host_resident.cpp  pht_gibbs_run_resident
 *   host_unif.cpp      what the uniformisation analyses share: staging (host_unif_plan.h), PhaseClock, grids
 *   host_loglik.cpp    log-likelihood blocks, pht_ctx_loglik* and pht_ctx_loglik_unif*
 *   host_predict.cpp   posterior-predictive replicates, pht_pred_* and pht_ctx_predict
 *   host_psis.cpp      PSIS-LOO: pht_ctx_loo_begin / _loo / _end (the fills are host_loglik.cpp's)
 *   host_estep.cpp     expected sufficient statistics: pht_ctx_estep, pht_estep_contract
 *   host_quantile.cpp  quantiles and residual-life quantiles: pht_ctx_quantile, pht_quantile_host
 *   host_fleet.cpp     what the three fleet calls share: the censored-unit list, pht_ctx_forecast_units, validators
 *   host_forecast.cpp  fleet forecasts of the censored units: pht_ctx_forecast, pht_forecast_host
 *   host_condition.cpp fleet condition of the censored units: pht_ctx_condition, pht_condition_host
 *   host_spares.cpp    fleet spares of the censored units: pht_ctx_spares, pht_spares_host
 *   host_replace.cpp   age-replacement policies: pht_ctx_replace, pht_replace_host
 */
#ifndef PHT_HOST_INTERNAL_H
#define PHT_HOST_INTERNAL_H

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdint.h>

#include <condition_variable>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/phasetype_amd.h"
#include "host_hip.h"
#include "host_lists.h"
#include "host_unif_plan.h"
#include "pht_kernels.h"
#include "pht_layout.h"
#include "pht_loglik_unif_args.h"
#include "rstream.h"

#pragma GCC visibility push(hidden)

namespace pht {
namespace host {

static_assert(kUnifRowsCap == kUnifMaxK, "unif_rows caps at the table's last row index");

/* ======================================================= error reporting */
/* the text behind pht_last_error: one object per thread, shared by every
 * unit (chain threads hand theirs to the caller, pht_gibbs_run_chains) */
extern thread_local std::string g_err;
void set_err(const char *fmt, ...);

#define HIPCHK(x)                                                               \
  do {                                                                          \
    hipError_t e_ = (x);                                                        \
    if (e_ != hipSuccess) {                                                     \
      ::pht::host::set_err("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
      return -1;                                                                \
    }                                                                           \
  } while (0)

/* ================================================ R runtime (when inside R) */
struct RHost {
  typedef double (*unif_fn)(void);
  typedef double (*rgamma_fn)(double, double);
  typedef void (*void_fn)(void);
  typedef void (*printf_fn)(const char *, ...);
  typedef void (*error_fn)(const char *, ...);
  bool inR = false;
  unif_fn unif = nullptr;
  rgamma_fn rgamma = nullptr;
  void_fn getrng = nullptr, putrng = nullptr, flush = nullptr;
  printf_fn rprintf = nullptr;
  error_fn rerror = nullptr;
  pht_rstream rs;
  bool seeded = false;
  RHost(); /* resolves R's functions when they are in the process */
  double u() { return inR ? unif() : pht_rs_unif_rand(&rs); }
  double gamma(double a, double sc) { return inR ? rgamma(a, sc) : pht_rs_rgamma(&rs, a, sc); }
  void begin() { if (inR) getrng(); }
  void end() { if (inR) putrng(); }
};
RHost &rhost();
void say(const char *fmt, ...);
/* a warning the caller must see: Rprintf inside R, stderr otherwise */
void warn(const char *fmt, ...);

/* a chain's own R-compatible stream (pht_gibbs_run_chains) */
struct OwnRng {
  pht_rstream rs;
  double u() { return pht_rs_unif_rand(&rs); }
  double gamma(double a, double sc) { return pht_rs_rgamma(&rs, a, sc); }
};

/* ============================================= parameters (host_params.cpp) */
bool lapack_ready();
/* the bound OpenBLAS on one thread for the duration of a scope (the
 * outermost one sets and restores: a Gibbs run once, a lone eigen() call
 * per call) */
struct OneBlasThread {
  int prev = 0;
  OneBlasThread();
  ~OneBlasThread();
};
/* evi_out: the eigenvalues' imaginary parts (the log-likelihood refuses a
 * complex spectrum, pht_loglik_build; the sampler goes on as the reference does) */
int eigen(int n, const double *S, double *evals, double *Q, double *Qinv, double *evi_out = nullptr);
int build_params(int n, const double *S, const double *s, int method, std::vector<unsigned char> &out);

/* the reference's precedence MHRS > DCS > ECS (src/PHT_MCMC_Aslett.c:325-337);
 * the opt-in uniformisation sampler (no reference counterpart) last */
inline int dispatch_method(int method) {
  if (method & kMethodMHRS) return kMethodMHRS;
  if (method & kMethodDCS) return kMethodDCS;
  if (method & kMethodECS) return kMethodECS;
  if (method & kMethodUNIF) return kMethodUNIF;
  return 0;
}

struct ChainGroup;

/* the device time of a call in two phases, summed over its batches: three
 * events (created on first use) and the two sums */
struct PhaseClock {
  Event ev[3];
  float ms[2] = {0.f, 0.f};
  int begin();                            /* a call starts: the events exist, the sums are zero */
  int mark(int i, hipStream_t st);        /* record event i */
  int add_after_sync();                   /* the batch is through: ms[0] += ev0..ev1, ms[1] += ev1..ev2 */
  float total() const { return ms[0] + ms[1]; }
};

}  // namespace host
}  // namespace pht

/* ========================================================== device context */
/* Member order is destruction order reversed: the streams come first, so
 * they are destroyed after every event and buffer below them (as
 * pht_ctx_destroy always did).  The holder selects the device first. */
struct pht_ctx {
  template <class T> using DevBuf = pht::host::DevBuf<T>;
  template <class T> using PinnedBuf = pht::host::PinnedBuf<T>;
  using Event = pht::host::Event;

  int device = 0;
  pht::host::Stream stream;
  /* ECS: the censored range runs on stream2, concurrently with the exact range */
  pht::host::Stream stream2;
  Event evf, evj;
  int n = 0, method = 0, mhit = 1;
  /* the reference method asked for (dispatch_method), and the path law of the
   * UNIF kernels when method is kMethodUNIF: 0 its own, 1 MHRS's / 2 DCS's
   * law by uniformisation (PHT_MHRS=bridge, PHT_DCS=bridge; pht_unif.h) */
  int rmethod = 0, ulaw = 0;
  long count = 0;
  long n_exact = 0;                      /* exact observations; ECS: positions [0, n_exact) (sorted first) */
  /* what pht_ctx_set_obs uploads and what is sized by it: replaced as a whole
   * by the next pht_ctx_set_obs */
  struct Obs {
    DevBuf<double> d_y;
    DevBuf<int> d_cens;
    DevBuf<uint32_t> d_gid;
    /* MHRS attempt-search workspace (count * (1 + mhit) tasks) */
    DevBuf<uint32_t> d_mbest, d_mq0, d_mq1;
    DevBuf<unsigned> d_mcnt;
    DevBuf<double> d_utab;               /* UNIF per-sweep table (pht_unif.h) */
    DevBuf<int> d_dcsb;                  /* DCS: per-position end states (dcs_end_kernel) */
    /* pht_ctx_loglik: the pointwise staging buffer, and the WAIC state per
     * observation in the device (sorted) order: 5 double arrays
     * [ref S1 S2 m r] and the counts */
    DevBuf<double> d_llpw;
    DevBuf<double> d_waic;
    DevBuf<long long> d_wcnt;
    /* pht_ctx_loo_*: the pointwise matrix [ndraws][count] in the device
     * (sorted) order, which rows a fill made usable, one transposed chunk
     * [chunk_obs][ndraws], the results [elpd khat lppd][count] and the flag
     * words; ndraws = 0: no pht_ctx_loo_begin yet */
    struct Loo {
      DevBuf<double> d_mat, d_chunk, d_out;
      DevBuf<int> d_flags, d_rows;
      int ndraws = 0;
      long chunk_obs = 0;
      std::vector<unsigned char> usable;
    } loo;
    /* pht_ctx_forecast: the censored units of these observations, listed on
     * first use (ncens < 0: not yet): their ages in the device (sorted) order,
     * unit -> the caller's observation index and -> its rank among the
     * censored observations in the caller's order, the largest age; a call's
     * state [unit][nh] (qsum, cnt) and one batch's pointwise values */
    struct Fcast {
      long ncens = -1;
      double ymax_c = 0.0;
      std::vector<long> idx, rank;
      DevBuf<double> d_age, d_qsum, d_q;
      DevBuf<int> d_cnt;
    } fc;
  } obs;
  DevBuf<unsigned char> d_params;
  DevBuf<unsigned long long> d_stats;
  PinnedBuf<unsigned long long> h_stats;
  PinnedBuf<unsigned char> h_params;
  std::vector<long> order;               /* sorted position -> local index */
  std::vector<double> h_ysorted;         /* y in device (sorted) order */
  double ysum = 0.0;                     /* sum of the shard's y (the fixed-point range check) */
  double ymax = 0.0;                     /* largest y of the shard (UNIF table length) */
  /* debug buffers (count observations each): allocated by the first debug
   * sweep, dropped by pht_ctx_set_obs */
  struct Dbg {
    DevBuf<long long> d_zq;
    DevBuf<int> d_N, d_B, d_pre, d_flags;
    DevBuf<uint32_t> d_ndraw;
  } dbg;
#ifdef PHT_BLOCK_TIMES
  /* variant builds: the ECS exact kernel's per-block records of the last
   * sweep (pht_kernels.h; pht_ctx_block_times), allocated by the first sweep */
  DevBuf<unsigned long long> d_blkt;
#endif
  float last_ms = 0.f;
  Event ev0, ev1;
  pht::host::ChainGroup *grp = nullptr; /* pht_gibbs_run_chains: exact ECS launched with the other chains */
  int gidx = -1;
  long long flagged = 0; /* flagged observation-sweeps of the last Gibbs run (node-wide) */
  long long global_count = -1; /* observations over all shards (pht_ctx_set_global_count) */
  ncclComm_t comm = nullptr; /* pht_ctx_attach_rccl: stats summed over ranks on `stream` (pht_ctx_destroy ends it) */
  DevBuf<long long> d_rccl; /* pht_ctx_rccl_prepare: staging buffer of pht_ctx_rccl_allreduce */
  int rccl_cap = 0;
  bool stats_zero = false;   /* d_stats zeroed on `stream` after the last sweep's copy */
  Event evd;                 /* the statistics copy to the host is done */
  /* the statistics block published by pht_stats_out_kernel: host-pinned
   * coherent words (mapped: .dev()) + a flag the host polls (empty: the copy
   * + event path, or PHT_STATS_COPY=1) */
  PinnedBuf<unsigned long long> h_out;
  PinnedBuf<unsigned> h_flag;
  unsigned seq = 0;
  /* sweeps enqueued and not yet waited for (oldest first): the statistics
   * flag value each publishes and its kernel-time event pair; two in flight
   * in the pipelined Gibbs loop (gibbs_run), else one */
  struct Inflight {
    unsigned seq = 0, gate = 0;
    bool timed = false;
    int evs = 0;
  } infl[2];
  int nin = 0;
  unsigned nenq = 0;
  Event ev0b, ev1b;
  /* the pipelined loop's gate (pht_gate_kernel): word 0 the released value
   * (host writes), word 16 the device's ack; the parameter block staged in
   * coherent pinned memory for the gate kernel's copy (both mapped) */
  PinnedBuf<unsigned> h_gate;
  PinnedBuf<unsigned char> h_pg;
  unsigned gate_seq = 0;
  int cus = 0; /* the device's CU count, read once (cu_count): the default grids derive from it */
  /* pht_ctx_loglik (allocated on first use): draw blocks and totals of a call */
  DevBuf<double> d_llblk;
  DevBuf<unsigned long long> d_lltot;
  /* pht_ctx_predict (allocated on first use; its own buffers, never the
   * sampler's): a call's tables + edges, flags, result words ([nd][8] sums,
   * [nd] ymin, [nd] ymax, [nd][ne + 1] counts) and one batch's pointwise
   * values and jump counts */
  DevBuf<double> d_predin, d_predy;
  DevBuf<int> d_predflag, d_prednj;
  DevBuf<unsigned long long> d_predout;
  /* pht_ctx_loglik_unif and the analyses below evaluate draws through the
   * uniformisation table and share its staging (host_unif.cpp): a call's (S, s,
   * meta words) in d_lluin and one batch's tables [draw][k][2] in d_llutab, the
   * context's own, never the sampler's obs.d_utab.  What each adds is allocated
   * on first use and its own too, never the sampler's or the WAIC state's;
   * X_grid_cap: 0 = the default grid (pht_ctx_X_grid_cap), X_clk: the last
   * call's device time. */
  DevBuf<double> d_lluin, d_llutab;
  /* pht_ctx_estep: one batch's int64 words [draw][class][k][G, T] and results
   * [draw][Z n, N n n, E n]; the totals are the log-likelihood's (d_lltot).
   * Default grid: one block a CU; clock: histograms (with the tables) and
   * contraction */
  DevBuf<long long> d_eswords;
  DevBuf<double> d_esout;
  int es_grid_cap = 0;
  pht::host::PhaseClock es_clk;
  /* pht_ctx_quantile: a call's sorted probabilities and horizons, one batch's
   * results [t, lo, hi][draw][p] and [nev, flags][draw][p].  Clock: tables
   * and searches */
  DevBuf<double> d_qin, d_qout;
  DevBuf<int> d_qouti;
  pht::host::PhaseClock q_clk;
  /* pht_ctx_forecast: a call's horizons and words [draw][horizon][4]; the
   * units and their state are obs.fc's.  Default grid: two blocks a CU; clock:
   * tables and evaluations */
  DevBuf<double> d_fch;
  DevBuf<unsigned long long> d_fcwords;
  int fc_grid_cap = 0;
  pht::host::PhaseClock fc_clk;
  /* pht_ctx_condition (never the forecast's buffers either): one batch's
   * forward tables [draw][k][n], a call's vectors [draw][m, r, scales] and
   * words [draw][n + nh + 3], the units' sums [unit][n + 2 + nh] and one
   * batch's pointwise values [unit][draw][n + 1 + nh]; the units are obs.fc's
   * (read only).  Default grid: two blocks a CU; clock: tables and units */
  DevBuf<double> d_cdF, d_cdvec, d_cdstate, d_cdpw;
  DevBuf<unsigned long long> d_cdwords;
  int cd_grid_cap = 0;
  pht::host::PhaseClock cd_clk;
  /* pht_ctx_spares (never the condition's buffers either): a call's horizons
   * and Kr per draw, one batch's forward tables [draw][k][n], weights
   * [draw][k][nh][T, p] and vectors [draw][r, q, scales], a call's words
   * [draw][2 nh + 2], the units' sums [unit][3 nh + 1] and one batch's pointwise
   * values [unit][draw][2 nh]; the units are obs.fc's (read only).  Default
   * grid: two blocks a CU; clock: vectors with the tables, and units */
  DevBuf<double> d_sph, d_spF, d_spW, d_spvec, d_spstate, d_sppw;
  DevBuf<int> d_spkr;
  DevBuf<unsigned long long> d_spwords;
  int sp_grid_cap = 0;
  pht::host::PhaseClock sp_clk;
  /* pht_ctx_replace (never the quantile's buffers either): a call's ages, cost
   * pairs, horizons and means, one batch's prefix sums [draw][K + 1], its curve
   * [lS, lf, M][draw][age] with the policies [t, g, lo, hi][draw][pair] and
   * the words [age flags][draw][age], [j, nev, flags][draw][pair].  Clock:
   * the tables with the curve, and the policies */
  DevBuf<double> d_rpin, d_rpcc, d_rpout;
  DevBuf<int> d_rpouti;
  pht::host::PhaseClock rp_clk;
};

namespace pht {
namespace host {

/* ================================================= context (host_ctx.cpp) */
/* the arguments every sweep launch of context c shares: its buffers, the
 * Philox key, the sweep number and the per-sweep knobs.  Each caller then
 * sets only what its launch differs in. */
SweepArgs sweep_args(pht_ctx *c, uint32_t k0, uint32_t k1, uint32_t sweep, int zexp);
/* ECS exact range: the claim-order knobs the one-context and the chains
 * launch share (PHT_NEWCAP, PHT_SPREAD; read per sweep) */
void ecs_claim_knobs(const pht_ctx *c, SweepArgs &ae);
/* UNIF: a's table fields for a largest lam of lmax, the context's table grown
 * to hold it (headroom: half as many rows again, for a host loop whose rates
 * move from sweep to sweep) */
int unif_table(pht_ctx *c, SweepArgs &a, double lmax, bool headroom);
int unif_prepare(pht_ctx *c, SweepArgs &a);
int ctx_launch(pht_ctx *c, const SweepArgs &a, bool debug);
int ctx_enqueue(pht_ctx *c, uint32_t k0, uint32_t k1, uint32_t sweep, int zexp, bool debug, bool timed = true,
                unsigned gate = 0);
int ctx_wait(pht_ctx *c);
void ctx_drain(pht_ctx *c);
void ctx_release(pht_ctx *c, unsigned gate, const unsigned char *pb, size_t bytes);

/* ================================ uniformisation analyses (host_unif.cpp) */
/* the context's CU count (at least 1), read from the device once; < 0: failed */
int cu_count(pht_ctx *c);
/* d_lluin and d_llutab hold plan p; S, s and its meta words go up on the
 * context's stream */
int unif_stage(pht_ctx *c, const UnifPlan &p, const double *S, const double *s);
/* the table kernel over the batch [d0, d0 + nb) of the staged plan; t: its
 * arguments (t.S, t.s, t.meta, t.tab are what the analysis' own kernels read) */
int unif_tables(pht_ctx *c, const UnifPlan &p, int d0, int nb, LlunifTableArgs &t);
/* the forward tables F [nb][fstride] of the same batch (pht_launch_cond_forward), rows a draw, after unif_tables */
int cond_forward(pht_ctx *c, const LlunifTableArgs &t, double *F, long fstride, int rows, int nb);
/* the bodies of pht_ctx_X_ms and pht_ctx_X_grid_cap (bad: the refusal's text after "who: ") */
int clock_read(const char *who, const pht_ctx *c, const PhaseClock pht_ctx::*clk, float *ms0, float *ms1);
int grid_cap_set(const char *who, const char *bad, pht_ctx *c, int pht_ctx::*cap, int value);

/* ======================= the censored units (host_fleet.cpp), as the
 * forecast, the condition and the spares take them */
/* the context's censored units listed (once per pht_ctx_set_obs), at least
 * one and at most max_units */
int censored_units(pht_ctx *c, const char *who, long max_units);
bool horizons_ok(const char *who, int nh, const double *h, int min_nh, int max_nh, int (*spec_ok)(int, const double *));
/* the _host twins' units: 1 <= ncens <= max_units; ymax_c 0 or finite and at
 * least the largest age (*ymax: the age the tables are sized for) */
bool units_ok(const char *who, long ncens, long max_units);
bool ymax_c_ok(const char *who, long ncens, const double *ages, double ymax_c, double *ymax);

/* =============================================== chains (host_chains.cpp) */
int group_sweep(pht_ctx *c, uint32_t k0, uint32_t k1, uint32_t sweep, int zexp);

/* ==================================================== RCCL (host_rccl.cpp) */
/*
 * RCCL bound at run time (dlopen), so the library loads where RCCL is absent
 * (inside R on a single GPU) and only multi-process runs need it.  Replaces
 * the per-sweep host callback (pht_reduce_fn) with an all-reduce on the device
 * copy of the statistics block, on the sweep's stream: no host round trip
 * between the kernels and the sum.  The reference has no distributed mode
 * (its observation loop is src/PHT_MCMC_Aslett.c:325-337).
 */
struct RcclApi {
  bool ok = false;
  ncclResult_t (*getUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*commInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*allReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
                            hipStream_t) = nullptr;
  ncclResult_t (*commDestroy)(ncclComm_t) = nullptr;
  const char *(*errStr)(ncclResult_t) = nullptr;
};
RcclApi &rccl();

/* ============================================ Gibbs loop (host_gibbs.cpp) */
/* Run the Gibbs loop over a set of device shards; reduce = optional
 * cross-process all-reduce of the int64 statistics block.  Rng: RHost or
 * OwnRng (instantiated in host_gibbs.cpp). */
template <class Rng>
int gibbs_run(Rng &R, int it, int method, int n, int m, const double *nu, const double *zeta, const int *T,
              const double *C, int silent, const double *start, double *res, std::vector<pht_ctx *> &ctxs,
              uint32_t k0, uint32_t k1, int zexp, pht_reduce_fn reduce, void *reduce_user, double *kernel_ms_total);

}  // namespace host
}  // namespace pht

#pragma GCC visibility pop

#endif
