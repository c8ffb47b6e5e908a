/*
 * host_lists.h — plain C++ (no HIP) pieces of the host runtime that the Gibbs
 * loop and the device-resident chain share: the per-parameter lists of the
 * structure matrices and the UNIF table length (tests/host/ checks both in a
 * stand-alone program).
 */
#ifndef PHT_HOST_LISTS_H
#define PHT_HOST_LISTS_H

#include <algorithm>
#include <cmath>
#include <vector>

#pragma GCC visibility push(hidden)
namespace pht {
namespace host {

struct Ent {
  int i, j;
  double c;
};

/* The reference's linked lists (src/PHT_MCMC_Aslett.c:214-262) as arrays in
 * insertion order: the walk over the (n+1)^2 matrices T and C runs i outer, j
 * inner; cell (i, j) with T[i + j n1] = k + 1 belongs to parameter k with
 * coefficient c = C[i + j n1].  (The reference visits its lists in reverse
 * insertion order; so do the users of these.) */
struct ParamLists {
  std::vector<std::vector<Ent>> Nl, Sl, sl, zl, TTl; /* [m] */
  std::vector<std::vector<Ent>> Dl;                  /* [n+1]: row i's cells */
  int bad_i = 0, bad_j = 0, bad_t = 0;               /* the rejected cell when build() fails */

  /* 0, or -1 for a T[i,j] outside 0..m (bad_* say which) */
  int build(int n, int m, const int *T, const double *C) {
    const int n1 = n + 1;
    for (auto *l : {&Nl, &Sl, &sl, &zl, &TTl}) l->assign(m, {});
    Dl.assign(n1, {});
    for (int i = 0; i < n1; i++)
      for (int j = 0; j < n1; j++) {
        const int t = T[i + j * n1];
        if (t == 0) continue;
        if (t < 1 || t > m) {
          bad_i = i;
          bad_j = j;
          bad_t = t;
          return -1;
        }
        const int k = t - 1;
        const double c = C[i + j * n1];
        if (j == n) { /* exit column: counted with the row's diagonal cell of N */
          Nl[k].push_back({i, i, 1.0});
          sl[k].push_back({i, 0, c});
        } else {
          Nl[k].push_back({i, j, 1.0});
          Sl[k].push_back({i, j, c});
        }
        zl[k].push_back({i, 0, c});
        TTl[k].push_back({i, j, c});
        Dl[i].push_back({i, j, 1.0});
      }
    return 0;
  }
};

/* UNIF: rows of the per-sweep table for a largest lam = mu y of lmax, with a
 * Poisson margin (pht_unif.h), capped at the table's last row index */
constexpr int kUnifRowsCap = 2047; /* = kUnifMaxK (pht_kernels.h; asserted in host_internal.h) */
inline int unif_rows(double lmax) {
  const double kd = std::ceil(lmax + 14.0 * std::sqrt(lmax) + 64.0);
  return (int)std::min<double>(kUnifRowsCap, std::isfinite(kd) ? kd : (double)kUnifRowsCap);
}

}  // namespace host
}  // namespace pht
#pragma GCC visibility pop

#endif
