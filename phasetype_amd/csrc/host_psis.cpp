/*
 * host_psis.cpp — PSIS-LOO cross-validation of the context's observations
 * (specification: include/pht_psis.h, kernels pht_psis.hip; no reference
 * counterpart).
 *
 * pht_ctx_loo_begin owns the pointwise matrix [ndraws][count] on the device;
 * the fills (host_loglik.cpp: the log-likelihood kernels as they are, pointed
 * at the matrix's rows) mark rows usable; pht_ctx_loo transposes the usable
 * rows chunk by chunk and runs one wavefront per observation.
 */
#include <string.h>

#include "host_internal.h"
#include "pht_psis.h"
#include "pht_psis_args.h"

using namespace pht;
using namespace pht::host;

/* the transposed chunk holds at most this many bytes (so it never doubles a
 * large matrix) and at least one observation */
static constexpr size_t kLooChunkBytes = (size_t)256 << 20;
/* free device memory left alone by pht_ctx_loo_begin: the log-likelihood
 * calls' own buffers and the runtime's */
static constexpr size_t kLooMarginBytes = (size_t)512 << 20;

static int loo_need(pht_ctx *c, const char *who, bool begun) {
  if (!c) {
    set_err("%s: null context", who);
    return -1;
  }
  if (c->count < 1 || !c->obs.d_y) {
    set_err("%s: no observations set on this context (pht_ctx_set_obs)", who);
    return -1;
  }
  if (begun && (c->obs.loo.ndraws < 1 || !c->obs.loo.d_mat)) {
    set_err("%s: no matrix on this context (pht_ctx_loo_begin)", who);
    return -1;
  }
  return 0;
}

extern "C" int pht_ctx_loo_begin(pht_ctx *c, int ndraws) {
  if (loo_need(c, "pht_ctx_loo_begin", false)) return -1;
  if (ndraws < 1 || ndraws > PHT_PSIS_MAXS) {
    set_err("pht_ctx_loo_begin: ndraws = %d outside 1..%d (thin the chain)", ndraws, PHT_PSIS_MAXS);
    return -1;
  }
  HIPCHK(hipSetDevice(c->device));
  ctx_drain(c);
  auto &L = c->obs.loo;
  L = pht_ctx::Obs::Loo{}; /* an earlier matrix goes first */
  const size_t count = (size_t)c->count, row = sizeof(double) * (size_t)ndraws;
  const size_t chunk_obs = std::min(count, std::max((size_t)1, kLooChunkBytes / row));
  const size_t need = row * count + row * chunk_obs + (3 * sizeof(double) + sizeof(int)) * count +
                      sizeof(int) * (size_t)ndraws;
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  if (need + kLooMarginBytes > free_b) {
    set_err("pht_ctx_loo_begin: the pointwise matrix of %d draws x %ld observations and its transposed chunk need "
            "%.1f MB, the device has %.1f MB free (a margin of %.0f MB is kept): thin the chain",
            ndraws, c->count, need / 1048576.0, free_b / 1048576.0, kLooMarginBytes / 1048576.0);
    return -1;
  }
  if (L.d_mat.alloc((size_t)ndraws * count) != hipSuccess || L.d_chunk.alloc((size_t)ndraws * chunk_obs) != hipSuccess ||
      L.d_out.alloc(3 * count) != hipSuccess || L.d_flags.alloc(count) != hipSuccess ||
      L.d_rows.alloc((size_t)ndraws) != hipSuccess) {
    (void)hipGetLastError();
    L = pht_ctx::Obs::Loo{};
    set_err("pht_ctx_loo_begin: allocating the pointwise matrix of %d draws x %ld observations failed: thin the chain",
            ndraws, c->count);
    return -1;
  }
  L.ndraws = ndraws;
  L.chunk_obs = (long)chunk_obs;
  L.usable.assign((size_t)ndraws, 0);
  return 0;
}

extern "C" int pht_ctx_loo(pht_ctx *c, double *elpd, double *khat, double *lppd, int *flags, int *ndraws_used) {
  if (loo_need(c, "pht_ctx_loo", true)) return -1;
  if (!elpd || !khat || !lppd || !flags) {
    set_err("pht_ctx_loo: null output");
    return -1;
  }
  auto &L = c->obs.loo;
  std::vector<int> rows;
  for (int d = 0; d < L.ndraws; d++)
    if (L.usable[d]) rows.push_back(d);
  const int S = (int)rows.size();
  if (ndraws_used) *ndraws_used = S;
  if (S < 1) {
    set_err("pht_ctx_loo: no usable draw among the matrix's %d rows (fill them: pht_ctx_loo_fill)", L.ndraws);
    return -1;
  }
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream.get();
  ctx_drain(c);
  const long count = c->count;
  int cus = 0;
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
  HIPCHK(hipMemcpyAsync(L.d_rows.get(), rows.data(), sizeof(int) * (size_t)S, hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(c->ev0.get(), st));
  for (long k0 = 0; k0 < count; k0 += L.chunk_obs) {
    const long kc = std::min(L.chunk_obs, count - k0);
    PsisTransposeArgs t{};
    t.mat = L.d_mat.get();
    t.count = count;
    t.rows = L.d_rows.get();
    t.S = S;
    t.k0 = k0;
    t.kc = kc;
    t.out = L.d_chunk.get();
    HIPCHK(pht_launch_psis_transpose(&t, st));
    PsisArgs a{};
    a.lt = L.d_chunk.get();
    a.S = S;
    a.kc = kc;
    a.elpd = L.d_out.get() + k0;
    a.khat = L.d_out.get() + count + k0;
    a.lppd = L.d_out.get() + 2 * count + k0;
    a.flags = L.d_flags.get() + k0;
    /* one wavefront a block, 19 KB of LDS each: eight a CU */
    HIPCHK(pht_launch_psis(&a, std::max(1, cus) * 8, st));
  }
  HIPCHK(hipEventRecord(c->ev1.get(), st));
  std::vector<double> h(3 * (size_t)count);
  std::vector<int> hf(count);
  HIPCHK(hipMemcpyAsync(h.data(), L.d_out.get(), sizeof(double) * 3 * (size_t)count, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hf.data(), L.d_flags.get(), sizeof(int) * (size_t)count, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipEventElapsedTime(&c->last_ms, c->ev0.get(), c->ev1.get()));
  for (long k = 0; k < count; k++) { /* back to the caller's observation order */
    const long o = c->order[k];
    elpd[o] = h[k];
    khat[o] = h[(size_t)count + k];
    lppd[o] = h[2 * (size_t)count + k];
    flags[o] = hf[k];
  }
  return 0;
}

extern "C" int pht_ctx_loo_end(pht_ctx *c) {
  if (!c) {
    set_err("pht_ctx_loo_end: null context");
    return -1;
  }
  HIPCHK(hipSetDevice(c->device));
  ctx_drain(c);
  HIPCHK(hipStreamSynchronize(c->stream.get()));
  c->obs.loo = pht_ctx::Obs::Loo{};
  return 0;
}
