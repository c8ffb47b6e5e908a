/*
 * host_unif.cpp — what the analyses that evaluate draws through the
 * uniformisation table share on the host (pht_ctx_loglik_unif, the PSIS fill,
 * pht_ctx_estep, _quantile, _forecast, _condition): the plan of a call
 * (host_unif_plan.h) staged on the device and its per-batch table launches, the
 * two-phase device clock, the CU count behind the default grids and the
 * bodies of the pht_ctx_X_ms / pht_ctx_X_grid_cap entry points.
 */
#include "host_internal.h"
#include "pht_condition_args.h"

using namespace pht;
using namespace pht::host;

int pht::host::cu_count(pht_ctx *c) {
  if (!c->cus) {
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    c->cus = std::max(1, cus);
  }
  return c->cus;
}

int pht::host::unif_stage(pht_ctx *c, const UnifPlan &p, const double *S, const double *s) {
  hipStream_t st = c->stream.get();
  HIPCHK(ensure(c->d_lluin, p.in_doubles()));
  HIPCHK(ensure(c->d_llutab, p.tab_doubles()));
  double *in = c->d_lluin.get();
  HIPCHK(hipMemcpyAsync(in + p.off_S(), S, sizeof(double) * p.nS, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(in + p.off_s(), s, sizeof(double) * p.ns, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(in + p.off_meta(), p.meta.data(), sizeof(double) * p.meta.size(), hipMemcpyHostToDevice, st));
  return 0;
}

int pht::host::unif_tables(pht_ctx *c, const UnifPlan &p, int d0, int nb, LlunifTableArgs &t) {
  const double *in = c->d_lluin.get();
  t = LlunifTableArgs{};
  t.n = p.n;
  t.nd = nb;
  t.S = in + p.off_S() + (size_t)d0 * p.n * p.n;
  t.s = in + p.off_s() + (size_t)d0 * p.n;
  t.meta = in + p.off_meta() + (size_t)d0 * PHT_LLU_META;
  t.tab = c->d_llutab.get();
  t.stride = p.stride;
  HIPCHK(pht_launch_llunif_table(&t, c->stream.get()));
  return 0;
}

int pht::host::cond_forward(pht_ctx *c, const LlunifTableArgs &t, double *F, long fstride, int rows, int nb) {
  CondTableArgs f{};
  f.n = t.n;
  f.nd = nb;
  f.S = t.S;
  f.meta = t.meta;
  f.F = F;
  f.fstride = fstride;
  f.rows = rows;
  HIPCHK(pht_launch_cond_forward(&f, c->stream.get()));
  return 0;
}

int PhaseClock::begin() {
  for (auto &e : ev)
    if (!e) HIPCHK(e.create());
  ms[0] = ms[1] = 0.f;
  return 0;
}

int PhaseClock::mark(int i, hipStream_t st) {
  HIPCHK(hipEventRecord(ev[i].get(), st));
  return 0;
}

int PhaseClock::add_after_sync() {
  float ms0 = 0.f, ms1 = 0.f;
  HIPCHK(hipEventElapsedTime(&ms0, ev[0].get(), ev[1].get()));
  HIPCHK(hipEventElapsedTime(&ms1, ev[1].get(), ev[2].get()));
  ms[0] += ms0;
  ms[1] += ms1;
  return 0;
}

int pht::host::clock_read(const char *who, const pht_ctx *c, const PhaseClock pht_ctx::*clk, float *ms0, float *ms1) {
  if (!c) {
    set_err("%s: null context", who);
    return -1;
  }
  if (ms0) *ms0 = (c->*clk).ms[0];
  if (ms1) *ms1 = (c->*clk).ms[1];
  return 0;
}

int pht::host::grid_cap_set(const char *who, const char *bad, pht_ctx *c, int pht_ctx::*cap, int value) {
  if (!c || value < 0) {
    set_err("%s: %s", who, bad);
    return -1;
  }
  c->*cap = value;
  return 0;
}
