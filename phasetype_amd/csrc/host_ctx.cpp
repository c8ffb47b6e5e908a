/*
 * host_ctx.cpp — the device context (pht_ctx) of one shard of observations:
 * create / destroy / pht_ctx_set_obs, and the sweep pipeline (enqueue the
 * sweep kernels of one parameter block on the context's streams, wait for its
 * statistics block).
 */
#include <math.h>
#include <sched.h>
#include <stdio.h>

#include <atomic>
#include <cmath>
#include <memory>
#include <numeric>

#include "host_internal.h"

using namespace pht;
using namespace pht::host;

/* lanes of the persistent ECS grid on an MI355X (256 CUs x 2 blocks x 256) */
constexpr long kSpreadLanes = 256L * 2 * 256;

extern "C" int pht_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

extern "C" pht_ctx *pht_ctx_create(int device, int n, int method, int mhit) {
  if (n < 1 || n > kMaxN) {
    set_err("n=%d outside 1..%d", n, kMaxN);
    return nullptr;
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) {
    set_err("no HIP device available (%s)", hipGetErrorString(e));
    return nullptr;
  }
  if (device < 0 || device >= ndev) {
    set_err("device %d out of range (%d devices)", device, ndev);
    return nullptr;
  }
  if (dispatch_method(method) == kMethodMHRS && (mhit < 0 || mhit > 1022)) {
    set_err("mhit=%d outside 0..1022 (MHRS attempt streams carry the chain index in 10 bits)", mhit);
    return nullptr;
  }
  std::unique_ptr<pht_ctx> c(new pht_ctx());
  c->device = device;
  c->n = n;
  c->method = c->rmethod = dispatch_method(method);
  c->mhit = mhit;
  /* bridge mode: MHRS or DCS path laws sampled exactly by the uniformisation
   * kernels (pht_unif.h) instead of the rejection search / Hobolth's
   * endpoint-conditioned sampler; same law, no eigensystem */
  if (c->rmethod == kMethodMHRS && env_is("PHT_MHRS", "bridge")) {
    c->method = kMethodUNIF;
    c->ulaw = 1;
  } else if (c->rmethod == kMethodDCS && env_is("PHT_DCS", "bridge")) {
    c->method = kMethodUNIF;
    c->ulaw = 2;
  }
  const size_t pb = make_layout(n).bytes(), sl = stats_len(n);
  /* (a failure frees what was created before it: c owns it all) */
  if (hipSetDevice(device) != hipSuccess || c->stream.create() != hipSuccess ||
      c->d_params.alloc(pb) != hipSuccess || c->d_stats.alloc(sl) != hipSuccess ||
      c->h_stats.alloc(sl) != hipSuccess || c->h_params.alloc(pb) != hipSuccess ||
      c->ev0.create() != hipSuccess || c->ev1.create() != hipSuccess || c->stream2.create() != hipSuccess ||
      c->evf.create_untimed() != hipSuccess || c->evj.create_untimed() != hipSuccess ||
      c->evd.create_untimed() != hipSuccess) {
    set_err("device %d: HIP allocation failed", device);
    return nullptr;
  }
  const unsigned fl = hipHostMallocCoherent | hipHostMallocMapped;
  /* the published statistics (optional: without them the copy + event path) */
  if (!getenv("PHT_STATS_COPY")) {
    if (c->h_out.alloc(sl, fl, true) == hipSuccess && c->h_flag.alloc(16, fl, true) == hipSuccess) {
      *c->h_flag.get() = 0u;
    } else {
      c->h_out.reset();
      c->h_flag.reset();
      (void)hipGetLastError();
    }
  }
  /* the pipelined loop's gate and staged parameters (optional: without them,
   * or with PHT_PIPELINE=0, the loop enqueues each sweep after the last) */
  if (c->h_out && !env_is("PHT_PIPELINE", "0")) {
    if (c->ev0b.create() == hipSuccess && c->ev1b.create() == hipSuccess &&
        c->h_gate.alloc(32, fl, true) == hipSuccess && c->h_pg.alloc(pb, fl, true) == hipSuccess) {
      c->h_gate.get()[0] = 0u;
      c->h_gate.get()[16] = 0u;
    } else {
      c->h_gate.reset();
      c->h_pg.reset();
      (void)hipGetLastError();
    }
  }
  return c.release();
}

extern "C" void pht_ctx_destroy(pht_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->comm && rccl().ok) (void)rccl().commDestroy(c->comm);
  delete c; /* buffers and events, then the streams (pht_ctx's member order) */
}

/* DCS end-state pre-pass from this many observations per shard */
constexpr long kDcsPrepassMin = 100000;

/*
 * Upload this shard's observations.  obs0 = global index of y[0]; the
 * Philox counter of observation i is obs0 + i whatever the shard layout.
 * Observations are reordered on the device (exact before censored, see
 * below); results do not depend on the order.
 */
extern "C" int pht_ctx_set_obs(pht_ctx *c, const double *y, const int *cens, long count, long obs0) {
  HIPCHK(hipSetDevice(c->device));
  /* everything of the previous observations goes: their arrays, the MHRS
   * workspace, the UNIF table, the DCS end states, the debug and the WAIC
   * buffers (capacities back to zero) */
  c->obs = pht_ctx::Obs{};
  c->dbg = pht_ctx::Dbg{};
  c->count = count;
  c->n_exact = 0;
  c->ysum = 0.0;
  c->ymax = 0.0;
  c->h_ysorted.clear();
  c->order.clear();
  if (count == 0) return 0;
  std::vector<long> ord(count);
  std::iota(ord.begin(), ord.end(), 0L);
  /* by decreasing y, so the persistent kernels hand out long paths first
   * and end on short ones (a short tail).  Exact observations first, then
   * censored ones, each by decreasing y: ECS runs the two as ranges of their
   * own (two kernels, two streams), and MHRS's and UNIF's code paths differ
   * for censored observations (a wavefront of one kind does not diverge).
   * DCS treats censored observations as exact (the reference's DCS law), so
   * its one kernel takes the whole shard by decreasing y (r04: the censored
   * range's long paths started two thirds of the way through the kernel and
   * set its tail; cfg5 DCS 1.19 -> 0.89 ms).  PHT_ORDER=asc|none: A/B of
   * ECS's exact range. */
  const bool split = !(c->method == kMethodDCS || (c->method == kMethodUNIF && c->ulaw == 2));
  const int omode = env_is("PHT_ORDER", "asc") ? 1 : (env_is("PHT_ORDER", "none") ? 2 : 0);
  std::stable_sort(ord.begin(), ord.end(), [&](long a, long b) {
    const int ca = cens[a] != 0, cb = cens[b] != 0;
    if (!split) return y[a] > y[b];
    if (ca != cb) return ca < cb;
    if (ca) return y[a] > y[b];
    if (omode == 2) return false;
    return omode == 1 ? (y[a] < y[b]) : (y[a] > y[b]);
  });
  std::vector<double> ys(count);
  std::vector<int> cs(count);
  std::vector<uint32_t> gs(count);
  for (long k = 0; k < count; k++) {
    ys[k] = y[ord[k]];
    cs[k] = cens[ord[k]];
    gs[k] = (uint32_t)(obs0 + ord[k]);
  }
  if (split) {
    while (c->n_exact < count && cs[c->n_exact] == 0) c->n_exact++;
  } else {
    for (long k = 0; k < count; k++) c->n_exact += (cs[k] == 0); /* (not a range here) */
  }
  c->h_ysorted = ys;
  for (double v : ys) {
    c->ysum += v;
    c->ymax = std::max(c->ymax, v);
  }
  c->order = std::move(ord);
  HIPCHK(c->obs.d_y.alloc(count));
  HIPCHK(c->obs.d_cens.alloc(count));
  HIPCHK(c->obs.d_gid.alloc(count));
  HIPCHK(hipMemcpy(c->obs.d_y.get(), ys.data(), sizeof(double) * count, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c->obs.d_cens.get(), cs.data(), sizeof(int) * count, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c->obs.d_gid.get(), gs.data(), sizeof(uint32_t) * count, hipMemcpyHostToDevice));
  if (c->method == kMethodMHRS) {
    const size_t tasks = (size_t)count * (size_t)(1 + c->mhit);
    HIPCHK(c->obs.d_mbest.alloc(tasks));
    HIPCHK(c->obs.d_mq0.alloc(tasks));
    HIPCHK(c->obs.d_mq1.alloc(tasks));
    HIPCHK(c->obs.d_mcnt.alloc(kMhrsCounters));
  }
  /* DCS: for large shards the end states come from a pre-pass kernel
   * (dcs_end_kernel; results identical).  Measured (profiles/r03/dcs_prepass/):
   * -4 % kernel time at n = 10, N = 10^6, -2 % at cfg5, flat at n = 5/20,
   * +6 % at N = 200 (one more launch).  PHT_DCS_PREPASS=1|0 forces it. */
  const bool pre = env_int("PHT_DCS_PREPASS", count >= kDcsPrepassMin) != 0;
  if (c->method == kMethodDCS && pre) HIPCHK(c->obs.d_dcsb.alloc(count));
  return 0;
}

/* exact observations (the longest, positions [0, k) of the decreasing-y
 * order) that run one per 16-lane row (pht_ecs_row.h) instead of one per
 * lane; PHT_ROWK=k forces k (results are identical for every k) */
static long exact_rowk(const pht_ctx *c) {
  if (const char *e = getenv("PHT_ROWK")) return std::max(0L, std::min(atol(e), c->n_exact));
  /* by exact observations per one-lane slot (kSpreadLanes ~ the resident
   * lanes of one MI355X); measured (tools/rowk_sweep.sh, tools/latency.py,
   * profiles/r02/rows): the fewer per lane, the more the longest paths set
   * the sweep time and the more rows pay (the launcher caps rows at half
   * the resident blocks) */
  const long L = kSpreadLanes;
  if (c->n_exact * 10 <= 6 * L) return 4096; /* 62.5k: 0.44 ms (1,024: 0.48; none: 0.56) */
  /* the 8-GPU shards of cfg4 (125k each, r04 kernels; profiles/r04/rowk):
   * max over the 8 real shards 0.487 ms at 2,048, 0.508 at 1,024, 0.498 at
   * 4,096, 0.517 at 512 */
  if (c->n_exact * 10 <= 12 * L) return 2048;
  /* the 4-GPU shards of cfg4 (250k each; r05 kernels, profiles/r05/shards_curve/): slowest shard
   * 0.621 / 0.621 / 0.630 ms at 4,096 against 0.641 / 0.627 / 0.641 at 1,024 (r02's kernels
   * preferred 1,024: 0.57 vs 0.59 ms) */
  if (c->n_exact <= 2 * L) return c->n == 10 ? 4096 : 1024; /* measured at n = 10 only: elsewhere r04's 1,024 */
  if (c->n_exact <= 5 * L) return 128;       /* cfg5's 350k exact: +5 % */
  return 0;                                  /* cfg4's 10^6: rows cost the one-lane range more (K = 64: +1 %) */
}

/* UNIF: size (and grow) the context's table for this sweep's parameters
 * (c->h_params): the shard's largest lam = mu y with a Poisson margin
 * (pht_unif.h).  Beyond kUnifMaxK rows or lam > kUnifMaxLam an observation
 * cannot be sampled exactly: it is counted in kXUnifCap and gibbs_run fails
 * the sweep */
int pht::host::unif_prepare(pht_ctx *c, SweepArgs &a) {
  const Layout L = make_layout(c->n);
  const double *S = reinterpret_cast<const double *>(c->h_params.get()) + L.S;
  double mu = 0.0;
  for (int i = 0; i < c->n; i++) mu = std::max(mu, -S[i + i * c->n]);
  if (!(mu > 0.0) || !std::isfinite(mu)) {
    set_err("UNIF: the generator's largest exit rate is %g (need a positive finite rate)", mu);
    return -1;
  }
  return unif_table(c, a, mu * c->ymax, true);
}

int pht::host::unif_table(pht_ctx *c, SweepArgs &a, double lmax, bool headroom) {
  a.uK = unif_rows(lmax);
  a.uymax = c->ymax;
  const long more = headroom ? unif_tab_doubles(c->n, std::min(kUnifMaxK, a.uK * 3 / 2)) : 0;
  HIPCHK(ensure(c->obs.d_utab, unif_tab_doubles(c->n, a.uK), more));
  a.utab = c->obs.d_utab.get();
  return 0;
}

SweepArgs pht::host::sweep_args(pht_ctx *c, uint32_t k0, uint32_t k1, uint32_t sweep, int zexp) {
  SweepArgs a;
  memset(&a, 0, sizeof a);
  a.params = c->d_params.get();
  a.n = c->n;
  a.mhit = c->mhit;
  a.ulaw = c->ulaw;
  a.count = c->count;
  a.y = c->obs.d_y.get();
  a.cens = c->obs.d_cens.get();
  a.gid = c->obs.d_gid.get();
  a.k0 = k0;
  a.k1 = k1;
  a.sweep = sweep;
  a.zscale = ldexp(1.0, zexp);
  /* DCS jump-time root finder: PHT_DCS_ROOT=brent selects the reference's
   * Find02 search (src/utility.c:233-338) over the default safeguarded Halley
   * iteration (pht_dcs_round.h hob_halley); read per sweep */
  a.dcsbrent = env_is("PHT_DCS_ROOT", "brent") ? 1 : 0;
  a.dcsb = c->obs.d_dcsb.get();
  a.stats = c->d_stats.get();
  a.mbest = c->obs.d_mbest.get();
  a.mq0 = c->obs.d_mq0.get();
  a.mq1 = c->obs.d_mq1.get();
  a.mcnt = c->obs.d_mcnt.get();
  return a;
}

void pht::host::ecs_claim_knobs(const pht_ctx *c, SweepArgs &ae) {
  /* one new observation per lane per round (PHT_NEWCAP=0: no limit;
   * tools/latency.py: -2 % kernel time at 1e6) */
  ae.newcap = env_int("PHT_NEWCAP", 1);
  /* lane-major first claims when the shard is within ~2 observations per
   * lane (the longest paths, one per wavefront; tools/latency.py:
   * -10 % at 31k-125k per GPU); PHT_SPREAD=0|1 forces it */
  ae.spread = env_int("PHT_SPREAD", c->n_exact <= 2 * kSpreadLanes);
  /* the share of a CU's older block against its younger one when the grid is
   * two one-lane blocks per CU (pair_pos, pht_claim.h): PHT_ECS_PAIR=43 | 32
   * for 4:3 | 3:2, 0 for the equal stripes; the launcher applies it only to
   * such a grid (no rows, no spread: the large shards).  On where it was
   * measured to pay (profiles/r14/ab/: kernel -6.9 % at cfg4, -8.4 % at
   * n = 5, 10^6); n = 15 at 10^6 is flat and n = 20 loses 4.6 %: the stripes */
  ae.pair = env_int("PHT_ECS_PAIR", (c->n == 5 || c->n == 10) ? 43 : 0);
}

/* the sweep kernels of one context on its stream(s): ECS exact and censored
 * ranges concurrently (stream2 joined back), the other samplers in one
 * launch; a carries the sweep's common arguments (ctx_enqueue, and the
 * resident chain per sweep) */
int pht::host::ctx_launch(pht_ctx *c, const SweepArgs &a, bool debug) {
  hipStream_t st = c->stream.get(), st2 = c->stream2.get();
  if (c->method == kMethodECS) {
    /* exact observations: persistent ECS kernel; censored: LJMA_samplechain path */
    SweepArgs ae = a;
    ae.begin = 0;
    ae.count = c->n_exact;
    ae.cens = nullptr;
    ae.occ = env_int("PHT_ECS_OCC", 0); /* blocks per CU of the persistent kernel (0: the occupancy limit) */
    ae.rowk = exact_rowk(c);
    ae.rowprio = env_int("PHT_ROWPRIO", 3);
    ecs_claim_knobs(c, ae);
    /* PHT_HOT=k: the remaining-time threshold is the k-th longest exact y */
    const long hk = env_long("PHT_HOT", 0);
    ae.hoty = (hk > 0 && hk <= c->n_exact) ? c->h_ysorted[hk - 1] : 0.0;
    SweepArgs ac = a;
    ac.begin = c->n_exact;
    ac.count = c->count - c->n_exact;
    ac.allcens = 1; /* positions [n_exact, count) hold the censored observations */
    /* both ranges: the censored kernel on stream2, concurrently, so each
     * persistent kernel's tail (its longest paths) fills with the other's
     * work; cfg5 ECS 2.49 -> 1.92 ms; the launch order does not matter
     * (PHT_CENS_SERIAL=1: one stream) */
    const bool fork = ae.count > 0 && ac.count > 0 && !getenv("PHT_CENS_SERIAL");
    /* n >= 15: the exact kernel's LDS now allows two blocks per CU (compact
     * parameter prefix, r04), which pays alone (n = 15, 5e5 exact: 1.178 ->
     * 1.038 ms) but crowds out the concurrent censored kernel (cfg5: 1.224
     * -> 1.482 ms; profiles/r04/ecs_lds/): with a censored range running
     * beside it, one block per CU as before */
    if (fork && c->n >= 15 && !getenv("PHT_ECS_OCC")) ae.occ = 1;
    if (fork) {
      HIPCHK(hipEventRecord(c->evf.get(), st));
      HIPCHK(hipStreamWaitEvent(st2, c->evf.get(), 0));
      HIPCHK(pht_launch_sweep(&ac, c->method, debug ? 1 : 0, st2));
      HIPCHK(hipEventRecord(c->evj.get(), st2));
      HIPCHK(pht_launch_sweep(&ae, c->method, debug ? 1 : 0, st));
      HIPCHK(hipStreamWaitEvent(st, c->evj.get(), 0));
    } else {
      if (ae.count > 0) HIPCHK(pht_launch_sweep(&ae, c->method, debug ? 1 : 0, st));
      if (ac.count > 0) HIPCHK(pht_launch_sweep(&ac, c->method, debug ? 1 : 0, st));
    }
  } else {
    HIPCHK(pht_launch_sweep(&a, c->method, debug ? 1 : 0, st));
  }
  return 0;
}

/* gate != 0: the pipelined loop's next sweep, enqueued while the current one
 * runs; its parameters come from c->h_pg once the host releases `gate`
 * (pht_gate_kernel), not from c->h_params now */
int pht::host::ctx_enqueue(pht_ctx *c, uint32_t k0, uint32_t k1, uint32_t sweep, int zexp, bool debug, bool timed,
                           unsigned gate) {
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream.get();
  if (c->nin >= 2 || (gate && (c->nin != 1 || !c->h_gate || !c->h_out))) {
    set_err("internal: sweep enqueued with %d in flight (gate %u)", c->nin, gate);
    return -1;
  }
  const int pb = make_layout(c->n).bytes();
  const int sl = stats_len(c->n);
  const int evs = (int)(c->nenq++ & 1u) && c->ev0b ? 1 : 0;
  hipEvent_t e0 = evs ? c->ev0b.get() : c->ev0.get(), e1 = evs ? c->ev1b.get() : c->ev1.get();
  if (gate) {
    HIPCHK(pht_launch_gate(c->h_gate.dev(), gate, reinterpret_cast<const unsigned long long *>(c->h_pg.dev()),
                           reinterpret_cast<unsigned long long *>(c->d_params.get()), pb / 8, c->h_gate.dev() + 16,
                           st));
  } else {
    HIPCHK(hipMemcpyAsync(c->d_params.get(), c->h_params.get(), pb, hipMemcpyHostToDevice, st));
  }
  /* the block is zeroed at the end of the previous sweep, after its copy to
   * the host (off the critical path: it runs while the host does the Gamma
   * update); only the first sweep, or one after a failed enqueue, zeroes it
   * here */
  if (!c->stats_zero) HIPCHK(hipMemsetAsync(c->d_stats.get(), 0, sizeof(unsigned long long) * sl, st));
  c->stats_zero = false;
  SweepArgs a = sweep_args(c, k0, k1, sweep, zexp);
  if (debug) {
    pht_ctx::Dbg &g = c->dbg;
    const size_t cnt = c->count, n = c->n;
    HIPCHK(ensure(g.d_zq, cnt * n));
    HIPCHK(ensure(g.d_N, cnt * n * n));
    HIPCHK(ensure(g.d_B, cnt));
    HIPCHK(ensure(g.d_pre, cnt));
    HIPCHK(ensure(g.d_flags, cnt));
    HIPCHK(ensure(g.d_ndraw, cnt));
    HIPCHK(hipMemsetAsync(g.d_zq.get(), 0, sizeof(long long) * cnt * n, st));
    HIPCHK(hipMemsetAsync(g.d_N.get(), 0, sizeof(int) * cnt * n * n, st));
    HIPCHK(hipMemsetAsync(g.d_B.get(), 0, sizeof(int) * cnt, st));
    HIPCHK(hipMemsetAsync(g.d_pre.get(), 0, sizeof(int) * cnt, st));
    a.dbg_zq = g.d_zq.get();
    a.dbg_N = g.d_N.get();
    a.dbg_B = g.d_B.get();
    a.dbg_pre = g.d_pre.get();
    a.dbg_flags = g.d_flags.get();
    a.dbg_ndraw = g.d_ndraw.get();
  }
#ifdef PHT_BLOCK_TIMES
  /* variant builds: the per-block records, zeroed ahead of the kernel-time
   * markers (a block that wrote nothing reads as zeros) */
  {
    const size_t words = (size_t)kBlkTimeCap * kBlkTimeWords;
    if (!c->d_blkt) HIPCHK(c->d_blkt.alloc(words));
    HIPCHK(hipMemsetAsync(c->d_blkt.get(), 0, sizeof(unsigned long long) * words, st));
    a.blk_times = c->d_blkt.get();
  }
#endif
  if (c->method == kMethodUNIF && unif_prepare(c, a)) return -1;
  /* the kernel-time markers: the GPU idles while the host enqueues them
   * (~9 us per sweep at cfg4, profiles/r06/kernel_events/), so the Gibbs loop
   * records them on a sample of its sweeps only */
  if (timed) HIPCHK(hipEventRecord(e0, st));
  if (ctx_launch(c, a, debug)) return -1;
  if (timed) HIPCHK(hipEventRecord(e1, st));
  if (c->comm) {
    /* multi-process: the block summed over all ranks in place, on the sweep's
     * stream, before the one copy to the host (pht_ctx_attach_rccl) */
    const ncclResult_t r =
        rccl().allReduce(c->d_stats.get(), c->d_stats.get(), (size_t)sl, ncclUint64, ncclSum, c->comm, st);
    if (r != ncclSuccess) {
      set_err("RCCL all-reduce of the statistics failed: %s", rccl().errStr(r));
      return -1;
    }
  }
  if (c->h_out) {
    /* one small kernel publishes the block and zeroes it; ctx_wait polls the
     * flag (kernel end -> host sees the statistics: the blit copy's dispatch,
     * its copy and the event's completion signal replaced by one dispatch and
     * a store over the link; profiles/r05/stats_out/) */
    if (++c->seq == 0u) c->seq = 1u;
    HIPCHK(pht_launch_stats_out(c->d_stats.get(), c->h_out.dev(), c->h_flag.dev(), c->seq, sl, st));
  } else {
    HIPCHK(hipMemcpyAsync(c->h_stats.get(), c->d_stats.get(), sizeof(unsigned long long) * sl, hipMemcpyDeviceToHost,
                          st));
    HIPCHK(hipEventRecord(c->evd.get(), st)); /* ctx_wait waits for this, not for the zeroing */
    HIPCHK(hipMemsetAsync(c->d_stats.get(), 0, sizeof(unsigned long long) * sl, st));
  }
  c->stats_zero = true;
  pht_ctx::Inflight &f = c->infl[c->nin++];
  f.seq = c->seq;
  f.gate = gate;
  f.timed = timed;
  f.evs = evs;
  return 0;
}

/* sweeps left in flight by an earlier call that failed: finish them and
 * forget their records (their statistics are stale), so the next wait
 * cannot take one of them for its own sweep */
void pht::host::ctx_drain(pht_ctx *c) {
  if (c->nin) {
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream.get());
    c->nin = 0;
    c->stats_zero = false;
  }
}

/* release the pipelined sweep waiting at `gate`: its parameter block (pb
 * bytes) into the staging buffer, then the gate word (release store; the
 * gate kernel's acquire load orders its copy after it) */
void pht::host::ctx_release(pht_ctx *c, unsigned gate, const unsigned char *pb, size_t bytes) {
  if (pb) memcpy(c->h_pg.get(), pb, bytes);
  __atomic_store_n(c->h_gate.get(), gate, __ATOMIC_RELEASE);
}

/* host threads inside wait_stats_flag right now: with more than one (several
 * chains driven from several threads, pht_gibbs_run_chains) a waiter yields
 * its core to the others' host work instead of pausing on it */
static std::atomic<int> g_stat_waiters{0};

static int wait_stats_flag_spin(pht_ctx *c, unsigned want) {
  for (unsigned long spin = 1;; spin++) {
    if (__atomic_load_n(c->h_flag.get(), __ATOMIC_ACQUIRE) == want) return 0;
    if (g_stat_waiters.load(std::memory_order_relaxed) > 1) sched_yield();
    if ((spin & 1023ul) == 0ul) {
      const hipError_t e = hipStreamQuery(c->stream.get());
      if (e == hipSuccess) {
        if (__atomic_load_n(c->h_flag.get(), __ATOMIC_ACQUIRE) == want) return 0;
        set_err("device %d: the sweep finished without publishing its statistics", c->device);
        return -1;
      }
      if (e != hipErrorNotReady) {
        set_err("device %d: %s", c->device, hipGetErrorString(e));
        return -1;
      }
    }
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
}

/* the flag pht_stats_out_kernel sets for this sweep; the stream is queried
 * now and then, so a failed or finished-without-flag sweep ends the wait */
static int wait_stats_flag(pht_ctx *c, unsigned want) {
  g_stat_waiters.fetch_add(1, std::memory_order_relaxed);
  const int rc = wait_stats_flag_spin(c, want);
  g_stat_waiters.fetch_sub(1, std::memory_order_relaxed);
  return rc;
}

/* the oldest sweep in flight: its statistics into c->h_stats, its kernel
 * time into c->last_ms (-1 when it was not timed) */
int pht::host::ctx_wait(pht_ctx *c) {
  HIPCHK(hipSetDevice(c->device));
  if (c->nin < 1) {
    set_err("internal: no sweep in flight");
    return -1;
  }
  const pht_ctx::Inflight f = c->infl[0];
  c->infl[0] = c->infl[1];
  c->nin--;
  hipEvent_t e0 = f.evs ? c->ev0b.get() : c->ev0.get(), e1 = f.evs ? c->ev1b.get() : c->ev1.get();
  if (c->h_out) {
    if (wait_stats_flag(c, f.seq)) return -1;
    memcpy(c->h_stats.get(), c->h_out.get(), sizeof(unsigned long long) * stats_len(c->n));
    if (f.gate && __atomic_load_n(c->h_gate.get() + 16, __ATOMIC_ACQUIRE) != f.gate) {
      set_err("device %d: a pipelined sweep's parameters were not released in time (gate %u, ack %u)", c->device,
              f.gate, __atomic_load_n(c->h_gate.get() + 16, __ATOMIC_ACQUIRE));
      return -1;
    }
    if (f.timed) {
      /* ev1 precedes the publishing kernel on the stream: it has completed */
      hipError_t e = hipEventElapsedTime(&c->last_ms, e0, e1);
      if (e == hipErrorNotReady) {
        HIPCHK(hipEventSynchronize(e1));
        e = hipEventElapsedTime(&c->last_ms, e0, e1);
      }
      HIPCHK(e);
    }
  } else {
    HIPCHK(hipEventSynchronize(c->evd.get()));
    if (f.timed) HIPCHK(hipEventElapsedTime(&c->last_ms, e0, e1));
  }
  if (!f.timed) c->last_ms = -1.f; /* not measured this sweep */
  if (c->method == kMethodMHRS && c->obs.d_mcnt && getenv("PHT_MHRS_COUNTS")) {
    /* diagnostics: tasks still unresolved after MHRS search rounds 0..4 */
    unsigned q[5];
    HIPCHK(hipMemcpy(q, c->obs.d_mcnt.get(), sizeof q, hipMemcpyDeviceToHost));
    fprintf(stderr, "[pht] MHRS unresolved after rounds 0-4: %u %u %u %u %u (of %ld tasks)\n", q[0], q[1], q[2],
            q[3], q[4], c->count * (1 + c->mhit));
  }
  return 0;
}

/* one sweep of (S, s), waited for: its statistics into stats_out */
static int sweep_once(pht_ctx *c, const double *S, const double *s, uint32_t k0, uint32_t k1, uint32_t sweep, int zexp,
                      bool debug, long long *stats_out) {
  std::vector<unsigned char> pb;
  int info = build_params(c->n, S, s, c->method, pb);
  if (info < 0) return info;
  memcpy(c->h_params.get(), pb.data(), pb.size());
  ctx_drain(c);
  if (ctx_enqueue(c, k0, k1, sweep, zexp, debug) || ctx_wait(c)) return -1;
  memcpy(stats_out, c->h_stats.get(), sizeof(long long) * stats_len(c->n));
  return 0;
}

extern "C" int pht_ctx_sweep(pht_ctx *c, const double *S, const double *s, uint32_t k0, uint32_t k1,
                             uint32_t sweep, int zexp, long long *stats_out) {
  return sweep_once(c, S, s, k0, k1, sweep, zexp, false, stats_out);
}

/* Per-observation debug sweep: outputs in the caller's original observation
 * order (B, pre, flags, ndraw [count]; zq [count*n]; N [count*n*n], N[i + j n]). */
extern "C" int pht_ctx_sweep_debug(pht_ctx *c, const double *S, const double *s, uint32_t k0, uint32_t k1,
                                   uint32_t sweep, int zexp, long long *stats_out, int *B, int *pre, int *flags,
                                   uint32_t *ndraw, long long *zq, int *N) {
  if (const int rc = sweep_once(c, S, s, k0, k1, sweep, zexp, true, stats_out)) return rc;
  const long cnt = c->count;
  const int n = c->n;
  std::vector<long long> hz(cnt * n);
  std::vector<int> hN(cnt * n * n), hB(cnt), hp(cnt), hf(cnt);
  std::vector<uint32_t> hd(cnt);
  HIPCHK(hipMemcpy(hz.data(), c->dbg.d_zq.get(), sizeof(long long) * cnt * n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hN.data(), c->dbg.d_N.get(), sizeof(int) * cnt * n * n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hB.data(), c->dbg.d_B.get(), sizeof(int) * cnt, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hp.data(), c->dbg.d_pre.get(), sizeof(int) * cnt, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hf.data(), c->dbg.d_flags.get(), sizeof(int) * cnt, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hd.data(), c->dbg.d_ndraw.get(), sizeof(uint32_t) * cnt, hipMemcpyDeviceToHost));
  for (long k = 0; k < cnt; k++) {
    const long o = c->order[k];
    B[o] = hB[k];
    pre[o] = hp[k];
    flags[o] = hf[k];
    ndraw[o] = hd[k];
    memcpy(zq + o * n, hz.data() + k * n, sizeof(long long) * n);
    memcpy(N + o * n * n, hN.data() + k * n * n, sizeof(int) * n * n);
  }
  return 0;
}

#ifdef PHT_BLOCK_TIMES
/* variant builds: the last sweep's per-block records (kBlkTimeWords words
 * each, pht_kernels.h) into out[cap * words]; returns the records copied */
extern "C" __attribute__((visibility("default"))) long pht_ctx_block_times(pht_ctx *c, unsigned long long *out,
                                                                           long cap, int *words) {
  if (words) *words = kBlkTimeWords;
  if (!c || !c->d_blkt || cap < 1) return 0;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream.get()));
  const long nrec = std::min<long>(cap, kBlkTimeCap);
  HIPCHK(hipMemcpy(out, c->d_blkt.get(), sizeof(unsigned long long) * (size_t)nrec * kBlkTimeWords,
                   hipMemcpyDeviceToHost));
  return nrec;
}
#endif
extern "C" float pht_ctx_last_kernel_ms(pht_ctx *c) { return c->last_ms; }
extern "C" long long pht_ctx_flagged_obs(pht_ctx *c) { return c->flagged; }
extern "C" int pht_ctx_set_global_count(pht_ctx *c, long long total) {
  if (!c || total < c->count) {
    set_err("pht_ctx_set_global_count: the total (%lld) must cover this shard's %ld observations", total,
            c ? c->count : 0L);
    return -1;
  }
  c->global_count = total;
  return 0;
}
