/*
 * host_unif_plan.h — the host arithmetic of one call of an analysis that
 * evaluates draws (S, s) through the uniformisation table
 * (include/pht_loglik_unif.h): the draws' meta words, the table stride of the
 * call, the batches and where S, s and the meta words lie in the input buffer.
 * Plain C++17, no HIP: host_unif.cpp puts it on the device, and
 * tests/host/unif_plan_check.cpp checks it alone.
 */
#ifndef PHT_HOST_UNIF_PLAN_H
#define PHT_HOST_UNIF_PLAN_H

#include <stddef.h>

#include <algorithm>
#include <vector>

#include "../../include/pht_loglik_unif.h"

namespace pht {
namespace host {

struct UnifPlan {
  int n, ndraws, batch;
  int Kcall = 0;            /* the largest K of the call */
  int stride, bmax;         /* table doubles a draw, 2 (Kcall + 1); draws of the largest batch */
  size_t nS, ns;            /* doubles of all S, of all s */
  std::vector<double> meta; /* [ndraws][PHT_LLU_META] */

  /* meta_of(d, Sd, sd, m) fills draw d's words m and returns its flag word
   * (pht_llu_meta, or an analysis' own on top of it); flags_out may be null */
  template <class MetaOf>
  UnifPlan(int n_, int ndraws_, const double *S, const double *s, int batch_, int *flags_out, MetaOf meta_of)
      : n(n_), ndraws(ndraws_), batch(batch_), nS((size_t)ndraws_ * n_ * n_), ns((size_t)ndraws_ * n_),
        meta((size_t)ndraws_ * PHT_LLU_META) {
    for (int d = 0; d < ndraws; d++) {
      double *m = meta.data() + (size_t)d * PHT_LLU_META;
      const unsigned flag = meta_of(d, S + (size_t)d * n * n, s + (size_t)d * n, m);
      if (flags_out) flags_out[d] = (int)flag;
      Kcall = std::max(Kcall, K(d));
    }
    stride = 2 * (Kcall + 1);
    bmax = std::min(batch, ndraws);
  }

  int K(int d) const { return (int)meta[(size_t)d * PHT_LLU_META + PHT_LLU_M_K]; }
  bool flagged(int d) const { return pht_d2u(meta[(size_t)d * PHT_LLU_META + PHT_LLU_M_FLAG]) != 0; }
  /* the largest K of the batch [d0, d0 + nb) */
  int Kmax(int d0, int nb) const {
    int k = 0;
    for (int d = d0; d < d0 + nb; d++) k = std::max(k, K(d));
    return k;
  }
  /* the input buffer [S | s | meta] and one batch's tables, in doubles */
  size_t off_S() const { return 0; }
  size_t off_s() const { return nS; }
  size_t off_meta() const { return nS + ns; }
  size_t in_doubles() const { return nS + ns + meta.size(); }
  size_t tab_doubles() const { return (size_t)bmax * stride; }
};

}  // namespace host
}  // namespace pht

#endif
