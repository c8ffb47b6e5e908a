/*
 * host_predict.cpp — posterior-predictive replicates of posterior draws.
 *
 * No reference counterpart.  Specification in include/pht_predict.h, kernel
 * pht_predict.hip.  pht_pred_build makes one draw's table on the host (no
 * device); pht_ctx_predict simulates nrep absorption times of PH(e_1, S_d) for
 * each draw on the context's stream and returns their exact integer
 * reductions, and in pointwise mode the times themselves.  Its buffers are the
 * context's own: no sampler or log-likelihood buffer is touched, and no
 * observations are needed.
 */
#include <math.h>
#include <string.h>

#include <cmath>
#include <limits>

#include "host_internal.h"
#include "pht_predict.h"
#include "pht_predict_args.h"

using namespace pht;
using namespace pht::host;

extern "C" int pht_pred_words(void) { return PHT_PRED_WORDS; }

extern "C" int pht_pred_table_words(int n) { return (n < 1 || n > PHT_PRED_MAXN) ? -1 : pht_pred_tab_words(n); }

extern "C" int pht_pred_build(int n, const double *S, const double *s, double *tab, int tab_words) {
  if (n < 1 || n > PHT_PRED_MAXN) {
    set_err("pht_pred_build: n = %d outside 1..%d", n, PHT_PRED_MAXN);
    return -1;
  }
  const int words = pht_pred_tab_words(n);
  if (!S || !s || !tab || tab_words < words) {
    set_err("pht_pred_build: null argument or tab_words < %d", words);
    return -2;
  }
  const unsigned flag = pht_pred_flags(n, S, s);
  if (flag)
    std::fill(tab, tab + words, 0.0);
  else
    pht_pred_table(n, S, s, tab);
  return (int)flag;
}

extern "C" int pht_ctx_predict(pht_ctx *c, int nd, const double *S, const double *s, int nrep, long long rep0,
                               unsigned draw0, unsigned k0, unsigned k1, double horizon, int max_jumps, int ne,
                               const double *edges, int batch, long long *words_out, long long *counts_out,
                               double *ymin_out, double *ymax_out, double *y_out, int *njump_out, int *flags_out) {
  const char *who = "pht_ctx_predict";
  if (!c) {
    set_err("%s: null context", who);
    return -1;
  }
  if (nd < 1 || !S || !s || !words_out || !counts_out || !ymin_out || !ymax_out || batch < 1 || batch > kPpredBatch) {
    set_err("%s: need nd >= 1, S, s, the four result arrays and 1 <= batch <= %d", who, kPpredBatch);
    return -1;
  }
  if (nrep < 1 || nrep > PHT_PRED_MAXREP) {
    set_err("%s: nrep = %d outside 1..%d (split a longer run by rep0)", who, nrep, PHT_PRED_MAXREP);
    return -1;
  }
  if (rep0 < 0 || rep0 + (long long)nrep > (1ll << 32)) {
    set_err("%s: rep0 + nrep = %lld beyond 2^32 replicate numbers", who, rep0 + (long long)nrep);
    return -1;
  }
  if ((unsigned long long)draw0 + (unsigned long long)nd > (1ull << 32)) {
    set_err("%s: draw0 + nd beyond 2^32 draw numbers", who);
    return -1;
  }
  if (ne < 0 || ne > PHT_PRED_MAXEDGES || (ne > 0 && !edges)) {
    set_err("%s: ne = %d outside 0..%d, or no edges", who, ne, PHT_PRED_MAXEDGES);
    return -1;
  }
  for (int k = 0; k < ne; k++)
    if (!std::isfinite(edges[k]) || (k > 0 && !(edges[k] > edges[k - 1]))) {
      set_err("%s: the edges must be finite and strictly increasing (edge %d)", who, k);
      return -1;
    }
  if (max_jumps < 1 || max_jumps > PHT_PRED_MAXJUMPS) {
    set_err("%s: max_jumps = %d outside 1..%d", who, max_jumps, PHT_PRED_MAXJUMPS);
    return -1;
  }
  if (!(horizon > 0.0)) {
    set_err("%s: the horizon must be positive (+inf: none)", who);
    return -1;
  }
  if (!y_out != !njump_out) {
    set_err("%s: pointwise mode needs both y_out and njump_out", who);
    return -1;
  }
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream.get();
  ctx_drain(c);
  const int n = c->n, tw = pht_pred_tab_words(n), nb1 = ne + 1;
  const bool pw = y_out != nullptr;

  /* the draws' tables and flags, then the edges */
  std::vector<double> hin((size_t)nd * tw + (size_t)ne, 0.0);
  std::vector<int> hflag(nd, 0);
  for (int d = 0; d < nd; d++) {
    const double *Sd = S + (size_t)d * n * n, *sd = s + (size_t)d * n;
    const unsigned flag = pht_pred_flags(n, Sd, sd);
    hflag[d] = (int)flag;
    if (!flag) pht_pred_table(n, Sd, sd, hin.data() + (size_t)d * tw);
    if (flags_out) flags_out[d] = (int)flag;
  }
  for (int k = 0; k < ne; k++) hin[(size_t)nd * tw + k] = edges[k];
  /* the results: [nd][8] words, [nd] ymin, [nd] ymax, [nd][ne + 1] counts */
  const size_t o_min = (size_t)nd * PHT_PRED_WORDS, o_max = o_min + nd, o_cnt = o_max + nd;
  std::vector<unsigned long long> hout(o_cnt + (size_t)nd * nb1, 0ull);
  for (int d = 0; d < nd; d++) hout[o_min + d] = 0x7ff0000000000000ull; /* +inf */

  const int bmax = std::min(batch, nd);
  HIPCHK(ensure(c->d_predin, hin.size()));
  HIPCHK(ensure(c->d_predflag, (size_t)nd));
  HIPCHK(ensure(c->d_predout, hout.size()));
  if (pw) {
    HIPCHK(ensure(c->d_predy, (size_t)bmax * (size_t)nrep));
    HIPCHK(ensure(c->d_prednj, (size_t)bmax * (size_t)nrep));
  }
  HIPCHK(hipMemcpyAsync(c->d_predin.get(), hin.data(), sizeof(double) * hin.size(), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->d_predflag.get(), hflag.data(), sizeof(int) * (size_t)nd, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->d_predout.get(), hout.data(), sizeof(unsigned long long) * hout.size(),
                        hipMemcpyHostToDevice, st));

  int cus = 0;
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
  /* device time of the call's launches (pointwise mode: with the copies
   * between them), read through pht_ctx_last_kernel_ms */
  HIPCHK(hipEventRecord(c->ev0.get(), st));
  for (int d0 = 0; d0 < nd; d0 += batch) {
    const int nb = std::min(batch, nd - d0);
    PpredArgs a{};
    a.n = n;
    a.nd = nb;
    a.nrep = (uint32_t)nrep;
    a.rep0 = (uint32_t)rep0;
    a.draw0 = draw0 + (uint32_t)d0;
    a.k0 = k0;
    a.k1 = k1;
    a.horizon = horizon;
    a.max_jumps = max_jumps;
    a.ne = ne;
    a.flags = c->d_predflag.get() + d0;
    a.tab = c->d_predin.get() + (size_t)d0 * tw;
    a.edges = c->d_predin.get() + (size_t)nd * tw;
    a.words = c->d_predout.get() + (size_t)d0 * PHT_PRED_WORDS;
    a.ymin = c->d_predout.get() + o_min + d0;
    a.ymax = c->d_predout.get() + o_max + d0;
    a.counts = c->d_predout.get() + o_cnt + (size_t)d0 * nb1;
    a.y = pw ? c->d_predy.get() : nullptr;
    a.nj = pw ? c->d_prednj.get() : nullptr;
    /* about ten blocks a CU over the launch (five are resident), at least one
     * and at most one per kPpredBlock replicates of a draw */
    const int want = (nrep + kPpredBlock - 1) / kPpredBlock;
    const int bpd = std::max(1, std::min(want, std::max(1, cus) * 10 / nb));
    HIPCHK(pht_launch_ppred(&a, bpd, st));
    if (pw) {
      const size_t cnt = (size_t)nb * (size_t)nrep;
      HIPCHK(hipMemcpyAsync(y_out + (size_t)d0 * nrep, c->d_predy.get(), sizeof(double) * cnt, hipMemcpyDeviceToHost,
                            st));
      HIPCHK(hipMemcpyAsync(njump_out + (size_t)d0 * nrep, c->d_prednj.get(), sizeof(int) * cnt,
                            hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      for (int d = 0; d < nb; d++) /* a flagged draw's block never ran */
        if (hflag[d0 + d])
          for (int r = 0; r < nrep; r++) {
            y_out[(size_t)(d0 + d) * nrep + r] = NAN;
            njump_out[(size_t)(d0 + d) * nrep + r] = 0;
          }
    }
  }
  HIPCHK(hipEventRecord(c->ev1.get(), st));
  HIPCHK(hipMemcpyAsync(hout.data(), c->d_predout.get(), sizeof(unsigned long long) * hout.size(),
                        hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipEventElapsedTime(&c->last_ms, c->ev0.get(), c->ev1.get()));
  memcpy(words_out, hout.data(), sizeof(long long) * o_min);
  memcpy(counts_out, hout.data() + o_cnt, sizeof(long long) * (size_t)nd * nb1);
  for (int d = 0; d < nd; d++) { /* no recorded replicate: the identities of min and max */
    const bool any = words_out[(size_t)d * PHT_PRED_WORDS + PHT_PRED_W_NDONE] > 0;
    double lo, hi;
    memcpy(&lo, &hout[o_min + d], 8);
    memcpy(&hi, &hout[o_max + d], 8);
    ymin_out[d] = any ? lo : std::numeric_limits<double>::infinity();
    ymax_out[d] = any ? hi : -std::numeric_limits<double>::infinity();
  }
  return 0;
}
