/*
 * host_resident.cpp — pht_gibbs_run_resident (opt-in, NON-PARITY): the whole
 * Gibbs loop on the device.  Per sweep the stream carries the step-1 kernels,
 * the optional RCCL all-reduce of the statistics, and resident_update_kernel
 * (pht_resident.hip: conjugate Gamma update by a counter-based sampler, the
 * next sweep's parameter block, the per-sweep checks); the host enqueues all
 * sweeps and waits once.  Every sampler: for ECS/DCS the update kernel also
 * builds the eigensystem (include/pht_eigen.h, one workgroup, in place of the
 * host's LAPACK dgeevx) and the spectral products.  The chain is a deterministic
 * function of the R stream's two key words (drawn at entry, as
 * pht_gibbs_run does) but NOT the host loop's chain (R's rgamma is replaced).
 */
#include <math.h>

#include <cmath>

#include "host_internal.h"

using namespace pht;
using namespace pht::host;

extern "C" int pht_gibbs_run_resident(pht_ctx *c, int it, int method, int m, const double *nu, const double *zeta,
                                      const int *T, const double *C, int zexp, const double *start, double *res,
                                      double *kernel_ms_total) {
  if (!c || it < 1 || m < 1 || m > (kMaxN + 1) * (kMaxN + 1)) {
    set_err("pht_gibbs_run_resident: need a context, it >= 1 and 1 <= m <= (kMaxN+1)^2");
    return -1;
  }
  if (dispatch_method(method) == 0 || dispatch_method(method) != c->rmethod) {
    set_err("pht_gibbs_run_resident: method %d needs a context created for that method (context %d)", method,
            c->rmethod);
    return -1;
  }
  const int disp = c->method; /* the kernels that run (UNIF for a bridge context) */
  if (!(ldexp(c->ysum, zexp) < 0x1p62)) {
    set_err("zexp = %d overflows the fixed-point z sums (the shard's observed times total %g)", zexp, c->ysum);
    return -1;
  }
  const int n = c->n, n1 = n + 1;
  RHost &R = rhost();
  R.begin();
  const uint32_t k0 = (uint32_t)(R.u() * 4294967296.0);
  const uint32_t k1 = (uint32_t)(R.u() * 4294967296.0);
  R.end();
  /* GibbsState's parameter lists (host_lists.h) as CSR, insertion order */
  ParamLists L;
  if (L.build(n, m, T, C)) {
    char why[160];
    L.describe(why, sizeof why);
    set_err("pht_gibbs_run_resident: %s", why);
    return -1;
  }
  std::vector<int> ints;   /* nl_off[m+1] nl_idx zl_off[m+1] zl_i tl_off[m+1] tl_ij dl_off[n+1] dl_ij */
  std::vector<double> dbl; /* nu[m] zeta[m] start[m] zl_c tl_c */
  /* the first `rows` lists of v: offsets, then each entry's index i + j ld */
  auto csr = [&](const std::vector<std::vector<Ent>> &v, int rows, int ld, int &off, int &idx) {
    off = (int)ints.size();
    int acc = 0;
    for (int r = 0; r < rows; r++) {
      ints.push_back(acc);
      acc += (int)v[r].size();
    }
    ints.push_back(acc);
    idx = (int)ints.size();
    for (int r = 0; r < rows; r++)
      for (const Ent &e : v[r]) ints.push_back(e.i + e.j * ld);
  };
  int o_nl, i_nl, o_zl, i_zl, o_tl, i_tl, o_dl, i_dl;
  csr(L.Nl, m, n, o_nl, i_nl); /* (an exit-column cell counts with the row's diagonal cell of N) */
  csr(L.zl, m, 0, o_zl, i_zl); /* the row i alone */
  csr(L.TTl, m, n1, o_tl, i_tl);
  csr(L.Dl, n, n1, o_dl, i_dl);
  dbl.insert(dbl.end(), nu, nu + m);
  dbl.insert(dbl.end(), zeta, zeta + m);
  const bool has_start = start && start[0] >= 0;
  for (int k = 0; k < m; k++) dbl.push_back(has_start ? start[k] : 0.0);
  const int o_zc = (int)dbl.size();
  for (int k = 0; k < m; k++)
    for (const Ent &e : L.zl[k]) dbl.push_back(e.c);
  const int o_tc = (int)dbl.size();
  for (int k = 0; k < m; k++)
    for (const Ent &e : L.TTl[k]) dbl.push_back(e.c);

  HIPCHK(hipSetDevice(c->device));
  DevBuf<int> bi, berr;
  DevBuf<double> bd, bres, btt;
  DevBuf<unsigned long long> bfl;
  HIPCHK(bi.alloc(ints.size()));
  HIPCHK(bd.alloc(dbl.size()));
  HIPCHK(bres.alloc((size_t)it * m));
  HIPCHK(btt.alloc((size_t)n1 * n1));
  HIPCHK(bfl.alloc(1));
  HIPCHK(berr.alloc(1));
  hipStream_t st = c->stream.get();
  HIPCHK(hipMemcpyAsync(bi.get(), ints.data(), sizeof(int) * ints.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(bd.get(), dbl.data(), sizeof(double) * dbl.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(btt.get(), 0, sizeof(double) * n1 * n1, st));
  HIPCHK(hipMemsetAsync(bfl.get(), 0, sizeof(unsigned long long), st));
  HIPCHK(hipMemsetAsync(berr.get(), 0, sizeof(int), st));
  HIPCHK(hipMemsetAsync(c->d_params.get(), 0, make_layout(n).bytes(), st));
  HIPCHK(hipMemsetAsync(c->d_stats.get(), 0, sizeof(unsigned long long) * stats_len(n), st));
  c->stats_zero = false;
  const int *di = bi.get();
  const double *dd = bd.get();
  ResidentArgs ra;
  memset(&ra, 0, sizeof ra);
  ra.n = n;
  ra.m = m;
  ra.it = it;
  ra.init = 1;
  ra.eig = (disp == kMethodECS || disp == kMethodDCS) ? 1 : 0;
  ra.unif = (disp == kMethodUNIF || c->ulaw) ? 1 : 0;
  ra.zs = ldexp(1.0, -zexp);
  ra.expect = c->global_count >= 0 ? c->global_count : (c->comm ? -1 : (long long)c->count);
  ra.k0 = k0;
  ra.k1 = k1;
  ra.nu = dd;
  ra.zeta = dd + m;
  ra.start = has_start ? dd + 2 * m : nullptr;
  ra.nl_off = di + o_nl;
  ra.nl_idx = di + i_nl;
  ra.zl_off = di + o_zl;
  ra.zl_i = di + i_zl;
  ra.zl_c = dd + o_zc;
  ra.tl_off = di + o_tl;
  ra.tl_ij = di + i_tl;
  ra.tl_c = dd + o_tc;
  ra.dl_off = di + o_dl;
  ra.dl_ij = di + i_dl;
  ra.stats = c->d_stats.get();
  ra.TT = btt.get();
  ra.res = bres.get();
  ra.params = c->d_params.get();
  ra.flagged = bfl.get();
  ra.err = berr.get();
  HIPCHK(pht_launch_resident_update(&ra, 0, st));
  ra.init = 0;

  SweepArgs a = sweep_args(c, k0, k1, 0, zexp); /* (sweep: set per iteration) */
  if (disp == kMethodUNIF) {
    /* table capacity: twice the prior mode's largest exit rate (the device
     * sizes each sweep's table from its own mu within it).  A chain whose mu
     * drifts past that needs rows beyond the capacity: those observations
     * are counted in kXUnifCap and the update kernel stops the run (err 16) */
    double mu0 = 0.0;
    for (int i = 0; i < n; i++) { /* row i's cells by increasing column (Dl[i]) */
      double rowsum = 0.0;
      for (const Ent &e : L.Dl[i]) {
        const int k = T[e.i + e.j * n1] - 1;
        const double th = has_start ? start[k] : (nu[k] > 1 ? (nu[k] - 1.0) / zeta[k] : nu[k] / zeta[k]);
        rowsum += th * C[e.i + e.j * n1];
      }
      mu0 = std::max(mu0, rowsum);
    }
    if (unif_table(c, a, 2.0 * mu0 * c->ymax, false)) return -1; /* (exact size: one table for the run) */
  }
  HIPCHK(hipEventRecord(c->ev0.get(), st));
  int early = 0; /* the error word, polled every kErrPoll sweeps */
  constexpr int kErrPoll = 256;
  for (int iter = 1; iter < it; iter++) {
    if (iter % kErrPoll == 0) {
      /* a failed sweep (e.g. the eigensystem) makes the update kernels
       * return at entry; stop enqueueing instead of running to `it`.  With a
       * communicator the decision is collective (the maximum of the ranks'
       * error words), so no rank leaves the loop while its peers still enter
       * the per-sweep all-reduce */
      if (c->comm && c->d_rccl) {
        HIPCHK(hipMemsetAsync(c->d_rccl.get(), 0, sizeof(long long), st));
        HIPCHK(hipMemcpyAsync(c->d_rccl.get(), berr.get(), sizeof(int), hipMemcpyDeviceToDevice, st));
        const ncclResult_t rr =
            rccl().allReduce(c->d_rccl.get(), c->d_rccl.get(), 1, ncclUint64, ncclMax, c->comm, st);
        if (rr != ncclSuccess) {
          set_err("RCCL all-reduce of the error word failed: %s", rccl().errStr(rr));
          return -1;
        }
        long long ew = 0;
        HIPCHK(hipMemcpyAsync(&ew, c->d_rccl.get(), sizeof ew, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        early = (int)ew;
      } else {
        HIPCHK(hipMemcpyAsync(&early, berr.get(), sizeof early, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
      }
      if (early) break;
    }
    a.sweep = (uint32_t)iter;
    if ((c->count > 0 || disp == kMethodUNIF) && ctx_launch(c, a, false)) return -1;
    if (c->comm) {
      const ncclResult_t rr =
          rccl().allReduce(c->d_stats.get(), c->d_stats.get(), (size_t)stats_len(n), ncclUint64, ncclSum, c->comm, st);
      if (rr != ncclSuccess) {
        set_err("RCCL all-reduce of the statistics failed: %s", rccl().errStr(rr));
        return -1;
      }
    }
    HIPCHK(pht_launch_resident_update(&ra, iter, st));
  }
  HIPCHK(hipEventRecord(c->ev1.get(), st));
  unsigned long long fl = 0;
  int err = 0;
  HIPCHK(hipMemcpyAsync(res, bres.get(), sizeof(double) * (size_t)it * m, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&fl, bfl.get(), sizeof fl, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&err, berr.get(), sizeof err, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, c->ev0.get(), c->ev1.get()));
  if (kernel_ms_total) *kernel_ms_total = ms;
  c->flagged = (long long)fl;
  if (err) {
    set_err("resident chain: %s%s%s%s%s", (err & 1) ? "a sweep did not sample every observation; " : "",
            (err & 2) ? "the fixed-point z sums overflowed (pass a smaller zexp); " : "",
            (err & 4) ? "a Gamma draw failed (non-finite shape/scale or the rejection cap); " : "",
            (err & 8) ? "the eigensystem failed (complex eigenvalues, no QR convergence, or a defective or nearly "
                        "defective S whose eigenvectors do not reproduce it:"
                        " the uniformisation sampler, method 8, needs none); " : "",
            (err & 16) ? "UNIF observations needed more uniformisation steps than the table sized from the start "
                         "(twice its largest exit rate) holds, or mu*y > 1300: the chain's rates drifted far above "
                         "the start (start nearer the posterior, or use the host loop, which sizes every sweep)" : "");
    return -1;
  }
  if (fl)
    warn("\nWARNING: %llu observation-sweeps hit a sampler cap or numerical guard in the resident chain\n", fl);
  return 0;
}
