/*
 * host_fleet.cpp — what the three fleet calls (host_forecast.cpp, _condition,
 * _spares) share: the list of the context's censored units, built once per
 * pht_ctx_set_obs, and the checks the device calls and their _host twins make.
 */
#include <math.h>

#include <algorithm>
#include <numeric>

#include "host_internal.h"
#include "pht_forecast.h"

using namespace pht;
using namespace pht::host;

bool pht::host::horizons_ok(const char *who, int nh, const double *h, int min_nh, int max_nh,
                            int (*spec_ok)(int, const double *)) {
  if (nh < min_nh || nh > max_nh || (nh > 0 && !h)) {
    set_err("%s: need %d <= nh <= %d horizons", who, min_nh, max_nh);
    return false;
  }
  if (!spec_ok(nh, h)) {
    set_err("%s: every horizon must be finite, >= 0 and larger than the one before", who);
    return false;
  }
  return true;
}

bool pht::host::units_ok(const char *who, long ncens, long max_units) {
  if (ncens < 1) {
    set_err("%s: no censored unit (ncens >= 1)", who);
    return false;
  }
  if (ncens > max_units) {
    set_err("%s: %ld censored units, at most %ld (the int64 sums)", who, ncens, max_units);
    return false;
  }
  return true;
}

bool pht::host::ymax_c_ok(const char *who, long ncens, const double *ages, double ymax_c, double *ymax) {
  double amax = 0.0;
  for (long i = 0; i < ncens; i++) amax = (ages[i] > amax) ? ages[i] : amax;
  if (ymax_c != 0.0 && !(ymax_c >= amax && ymax_c < INFINITY)) {
    set_err("%s: ymax_c must be 0 (the largest age) or finite and at least the largest age", who);
    return false;
  }
  *ymax = ymax_c != 0.0 ? ymax_c : amax;
  return true;
}

namespace {

/* the censored units of the context's observations, listed once per
 * pht_ctx_set_obs: ages in the device order, the caller's index and rank */
int forecast_units(pht_ctx *c, const char *who) {
  if (!c) {
    set_err("%s: null context", who);
    return -1;
  }
  auto &fc = c->obs.fc;
  if (fc.ncens >= 0) return 0;
  if (c->count < 1 || !c->obs.d_y) {
    fc.ncens = 0;
    return 0;
  }
  HIPCHK(hipSetDevice(c->device));
  ctx_drain(c);
  std::vector<int> cens((size_t)c->count);
  HIPCHK(hipMemcpy(cens.data(), c->obs.d_cens.get(), sizeof(int) * (size_t)c->count, hipMemcpyDeviceToHost));
  std::vector<double> ages;
  fc.idx.clear();
  fc.ymax_c = 0.0;
  for (long k = 0; k < c->count; k++) {
    if (!cens[k]) continue;
    ages.push_back(c->h_ysorted[k]);
    fc.idx.push_back(c->order[k]);
    fc.ymax_c = std::max(fc.ymax_c, c->h_ysorted[k]);
  }
  const long nc = (long)ages.size();
  std::vector<long> by(nc);
  std::iota(by.begin(), by.end(), 0L);
  std::sort(by.begin(), by.end(), [&](long x, long y) { return fc.idx[x] < fc.idx[y]; });
  fc.rank.assign(nc, 0);
  for (long r = 0; r < nc; r++) fc.rank[by[r]] = r;
  if (nc > 0 && nc <= PHT_FC_MAXUNITS) {
    HIPCHK(fc.d_age.alloc((size_t)nc));
    HIPCHK(hipMemcpy(fc.d_age.get(), ages.data(), sizeof(double) * (size_t)nc, hipMemcpyHostToDevice));
  }
  fc.ncens = nc;
  return 0;
}

}  // namespace

int pht::host::censored_units(pht_ctx *c, const char *who, long max_units) {
  if (forecast_units(c, who)) return -1;
  const long ncens = c->obs.fc.ncens;
  if (ncens < 1) {
    set_err("%s: no censored observation on this context (pht_ctx_set_obs)", who);
    return -1;
  }
  if (ncens > max_units) {
    set_err("%s: %ld censored units on this context, at most %ld (the int64 sums): shard them", who, ncens, max_units);
    return -1;
  }
  return 0;
}

extern "C" long pht_ctx_forecast_units(pht_ctx *c, long *idx_out) {
  if (forecast_units(c, "pht_ctx_forecast_units")) return -1;
  const auto &fc = c->obs.fc;
  if (idx_out)
    for (long u = 0; u < fc.ncens; u++) idx_out[fc.rank[u]] = fc.idx[u];
  return fc.ncens;
}
