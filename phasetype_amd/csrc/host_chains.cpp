/*
 * host_chains.cpp — several independent chains on one device whose sweeps go
 * out together (ChainGroup), and pht_gibbs_run_chains.
 */
#include <math.h>

#include <thread>

#include "host_internal.h"

using namespace pht;
using namespace pht::host;

/*
 * Chains whose sweeps go out together (pht_gibbs_run_chains, SURVEY.md
 * §8f.4).  Each chain's thread builds its parameters into its slot of one
 * pinned block and arrives; the last chain to arrive enqueues the whole sweep
 * of every arrived chain on the group's stream: one parameter upload, one
 * statistics reset, ONE ecs_chains_kernel launch over all exact ranges (the
 * censored-range kernels concurrently on stream2), one statistics
 * download.  The others wait for that sweep's `done` event.  A chain that
 * stops (end of run or error) leaves the group, so the others never wait
 * for it.
 */
struct pht::host::ChainGroup {
  int K = 0, device = 0, n = 0, pb = 0, sl = 0, method = kMethodECS;
  /* (the streams first: destroyed last, after the events and buffers) */
  Stream stream;
  /* censored ranges run on stream2, concurrently with the exact-range launch */
  Stream stream2;
  std::mutex m;
  std::condition_variable cv;
  int active = 0;
  unsigned long gen = 0;
  int rc = 0;
  float ms = 0.f;
  std::vector<int> who;          /* chains arrived for the pending sweep */
  std::vector<SweepArgs> ex, ce; /* [K] exact / censored range arguments */
  PinnedBuf<unsigned char> h_params;       /* [K][pb] */
  DevBuf<unsigned char> d_params;
  PinnedBuf<unsigned long long> h_stats;   /* [K][sl] */
  DevBuf<unsigned long long> d_stats;
  PinnedBuf<SweepArgs> h_args;             /* [2K] packed: exact ranges, then censored ranges */
  DevBuf<SweepArgs> d_args;
  Event ev0, ev1, done;
  Event evf, evj;
};

static void group_destroy(ChainGroup *g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  if (g->stream) (void)hipStreamSynchronize(g->stream.get());
  if (g->stream2) (void)hipStreamSynchronize(g->stream2.get());
  delete g;
}

static ChainGroup *group_create(int device, int K, int n, int method) {
  ChainGroup *g = new ChainGroup();
  g->K = K;
  g->method = method;
  g->device = device;
  g->n = n;
  g->pb = make_layout(n).bytes();
  g->sl = stats_len(n);
  g->active = K;
  g->ex.resize(K);
  g->ce.resize(K);
  const size_t P = (size_t)g->pb * K, S = (size_t)g->sl * K, A = 2 * (size_t)K;
  const bool ok = hipSetDevice(device) == hipSuccess && g->stream.create() == hipSuccess &&
                  g->ev0.create() == hipSuccess && g->ev1.create() == hipSuccess &&
                  g->done.create_untimed() == hipSuccess && g->stream2.create() == hipSuccess &&
                  g->evf.create_untimed() == hipSuccess && g->evj.create_untimed() == hipSuccess &&
                  g->h_params.alloc(P) == hipSuccess && g->d_params.alloc(P) == hipSuccess &&
                  g->h_stats.alloc(S) == hipSuccess && g->d_stats.alloc(S) == hipSuccess &&
                  g->h_args.alloc(A) == hipSuccess && g->d_args.alloc(A) == hipSuccess;
  if (!ok) {
    group_destroy(g);
    return nullptr;
  }
  return g;
}

/* with g->m held: enqueue the sweep of the arrived chains and release them */
static void group_fire(ChainGroup *g) {
  const int k = (int)g->who.size();
  hipStream_t st = g->stream.get(), st2 = g->stream2.get();
  SweepArgs *ha = g->h_args.get(), *da = g->d_args.get();
  const size_t sbytes = sizeof(unsigned long long) * g->sl * g->K;
  hipError_t e = hipSetDevice(g->device);
  if (e == hipSuccess)
    e = hipMemcpyAsync(g->d_params.get(), g->h_params.get(), (size_t)g->pb * g->K, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(g->d_stats.get(), 0, sbytes, st);
  if (e == hipSuccess) e = hipEventRecord(g->ev0.get(), st);
  int nx = 0, nc = 0;
  if (g->method == kMethodECS) {
    /* exact ranges [0, K), censored ranges [K, 2K) of the packed arguments */
    for (int i = 0; i < k; i++) {
      const int w = g->who[i];
      if (g->ex[w].count > 0) ha[nx++] = g->ex[w];
    }
    for (int i = 0; i < k; i++) {
      const int w = g->who[i];
      if (g->ce[w].count > 0) ha[g->K + nc++] = g->ce[w];
    }
  } else {
    for (int i = 0; i < k; i++)
      if (g->ex[g->who[i]].count > 0) ha[nx++] = g->ex[g->who[i]];
  }
  if (e == hipSuccess) e = hipMemcpyAsync(da, ha, sizeof(SweepArgs) * 2 * g->K, hipMemcpyHostToDevice, st);
  /* ECS: every chain's censored range in one launch on stream2 while the
   * exact ranges run (as ctx_enqueue) */
  const bool fork = nc > 0 && nx > 0;
  if (e == hipSuccess && fork) e = hipEventRecord(g->evf.get(), st);
  if (e == hipSuccess && fork) e = hipStreamWaitEvent(st2, g->evf.get(), 0);
  if (e == hipSuccess && nc > 0) e = pht_launch_chains(ha + g->K, da + g->K, nc, kMethodECS, fork ? st2 : st);
  if (e == hipSuccess && fork) e = hipEventRecord(g->evj.get(), st2);
  if (e == hipSuccess && nx > 0)
    e = g->method == kMethodECS ? pht_launch_ecs_chains(ha, da, nx, st)
                                : pht_launch_chains(ha, da, nx, g->method, st);
  if (e == hipSuccess && fork) e = hipStreamWaitEvent(st, g->evj.get(), 0);
  if (e == hipSuccess) e = hipEventRecord(g->ev1.get(), st);
  if (e == hipSuccess) e = hipMemcpyAsync(g->h_stats.get(), g->d_stats.get(), sbytes, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipEventRecord(g->done.get(), st);
  g->rc = (e == hipSuccess) ? 0 : (int)e;
  g->who.clear();
  g->gen++;
  g->cv.notify_all();
}

/* chain c's sweep (parameters in c->h_params): returns when the group's sweep
 * is done, with c->h_stats and c->last_ms filled */
int pht::host::group_sweep(pht_ctx *c, uint32_t k0, uint32_t k1, uint32_t sweep, int zexp) {
  ChainGroup *g = c->grp;
  const int w = c->gidx;
  /* the group's block and statistics slot of this chain; what depends on the
   * range is set per range below */
  SweepArgs a = sweep_args(c, k0, k1, sweep, zexp);
  a.params = g->d_params.get() + (size_t)g->pb * w;
  a.stats = g->d_stats.get() + (size_t)g->sl * w;
  a.count = 0;
  a.cens = nullptr;
  a.dcsb = nullptr; /* the chains launch computes the end states in its round kernel */
  a.mbest = a.mq0 = a.mq1 = nullptr;
  a.mcnt = nullptr;
  SweepArgs ae = a, ac = a;
  if (g->method == kMethodECS) {
    ae.begin = 0;
    ae.count = c->n_exact;
    ecs_claim_knobs(c, ae);
    ac.cens = c->obs.d_cens.get();
    ac.begin = c->n_exact;
    ac.count = c->count - c->n_exact;
    ac.allcens = 1;
  } else {
    /* the whole shard in one argument (MHRS, DCS, UNIF) */
    ae.begin = 0;
    ae.count = c->count;
    ae.cens = c->obs.d_cens.get();
    ae.mbest = c->obs.d_mbest.get();
    ae.mq0 = c->obs.d_mq0.get();
    ae.mq1 = c->obs.d_mq1.get();
    ae.mcnt = c->obs.d_mcnt.get();
    if (g->method == kMethodUNIF && unif_prepare(c, ae)) return -1;
    ac.count = 0;
  }
  std::unique_lock<std::mutex> lk(g->m);
  memcpy(g->h_params.get() + (size_t)g->pb * w, c->h_params.get(), g->pb);
  g->ex[w] = ae;
  g->ce[w] = ac;
  g->who.push_back(w);
  const unsigned long my = g->gen;
  if ((int)g->who.size() == g->active) group_fire(g);
  else g->cv.wait(lk, [&] { return g->gen != my; });
  const int rc = g->rc; /* the next sweep needs this chain's arrival: rc is still ours */
  lk.unlock();
  if (rc) {
    set_err("chains sweep enqueue failed (%s)", hipGetErrorString((hipError_t)rc));
    return -1;
  }
  HIPCHK(hipEventSynchronize(g->done.get()));
  HIPCHK(hipEventElapsedTime(&c->last_ms, g->ev0.get(), g->ev1.get()));
  memcpy(c->h_stats.get(), g->h_stats.get() + (size_t)g->sl * w, sizeof(unsigned long long) * g->sl);
  return 0;
}

static void group_leave(ChainGroup *g) {
  std::lock_guard<std::mutex> lk(g->m);
  g->active--;
  if (!g->who.empty() && (int)g->who.size() == g->active) group_fire(g);
}

/*
 * Several independent chains at once: chain c runs on its
 * own context (device buffers and HIP stream) from a host thread of its own,
 * with its own R-compatible stream seeded by seeds[c] (standalone mode: the
 * Gamma draws and the Philox key come from it), so chain c is exactly the
 * single-chain pht_gibbs_run after pht_set_seed(seeds[c]).  At small N each
 * chain's kernels leave most of the GPU idle (their time is the longest
 * latent path); the chains' kernels run concurrently on their streams and the
 * host setups overlap.  res is [chain][it x m] (each block as pht_gibbs_run);
 * start is [chain][m] or start[0] < 0.  Not for use inside R (threads).
 */
extern "C" int pht_gibbs_run_chains(pht_ctx **ctxs, int nchains, const uint32_t *seeds, int it, int method, int m,
                                    const double *nu, const double *zeta, const int *T, const double *C, int zexp,
                                    const double *start, double *res, double *kernel_ms_max) {
  if (nchains < 1 || !ctxs || !seeds) {
    set_err("pht_gibbs_run_chains: need nchains >= 1 contexts and seeds");
    return -1;
  }
  if (rhost().inR) {
    set_err("pht_gibbs_run_chains is not available inside R (host threads)");
    return -1;
  }
  for (int c = 0; c < nchains; c++)
    if (!ctxs[c] || ctxs[c]->comm) {
      set_err("pht_gibbs_run_chains: context %d is null or has an RCCL communicator attached", c);
      return -1;
    }
  /* all chains' sweeps in one launch sequence, when the chains share a
   * device, n and method (ECS: the exact ranges in one ecs_chains_kernel and
   * the censored ranges in one cens_chains_kernel; MHRS/DCS/UNIF: one
   * launch_chains sequence); PHT_CHAINS_LAUNCH=streams: a launch per chain */
  ChainGroup *grp = nullptr;
  {
    bool one = nchains >= 2;
    for (int c = 0; c < nchains && one; c++)
      one = ctxs[c]->method == ctxs[0]->method && ctxs[c]->ulaw == ctxs[0]->ulaw &&
            ctxs[c]->device == ctxs[0]->device && ctxs[c]->n == ctxs[0]->n && !ctxs[c]->grp;
    if (env_is("PHT_CHAINS_LAUNCH", "streams")) one = false;
    if (one) {
      grp = group_create(ctxs[0]->device, nchains, ctxs[0]->n, ctxs[0]->method);
      if (!grp) {
        set_err("pht_gibbs_run_chains: HIP allocation failed");
        return -1;
      }
      for (int c = 0; c < nchains; c++) {
        ctxs[c]->grp = grp;
        ctxs[c]->gidx = c;
      }
    }
  }
  std::vector<int> rc(nchains, 0);
  std::vector<double> kms(nchains, 0.0);
  std::vector<std::string> err(nchains);
  std::vector<std::thread> th;
  for (int c = 0; c < nchains; c++) {
    th.emplace_back([&, c]() {
      OwnRng R;
      pht_rs_set_seed(&R.rs, seeds[c]);
      const uint32_t k0 = (uint32_t)(R.u() * 4294967296.0);
      const uint32_t k1 = (uint32_t)(R.u() * 4294967296.0);
      std::vector<pht_ctx *> one{ctxs[c]};
      const double *st = (start && start[0] >= 0) ? start + (size_t)c * m : start;
      rc[c] = gibbs_run(R, it, method, ctxs[c]->n, m, nu, zeta, T, C, 1, st, res + (size_t)c * it * m, one, k0, k1,
                        zexp, nullptr, nullptr, &kms[c]);
      if (rc[c]) err[c] = g_err;
      if (grp) group_leave(grp);
    });
  }
  for (auto &t : th) t.join();
  if (grp) {
    for (int c = 0; c < nchains; c++) {
      ctxs[c]->grp = nullptr;
      ctxs[c]->gidx = -1;
    }
    group_destroy(grp);
  }
  double mx = 0.0;
  for (int c = 0; c < nchains; c++) {
    if (rc[c]) {
      set_err("chain %d: %s", c, err[c].c_str());
      return -1;
    }
    mx = std::max(mx, kms[c]);
  }
  if (kernel_ms_max) *kernel_ms_max = mx;
  return 0;
}
