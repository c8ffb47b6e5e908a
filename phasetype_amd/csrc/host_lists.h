/*
 * host_lists.h — plain C++ (no HIP) pieces of the host runtime that the Gibbs
 * loop and the device-resident chain share: the per-parameter lists of the
 * structure matrices and the UNIF table length (tests/host/ checks both in a
 * stand-alone program), and the Gibbs bookkeeping itself (GibbsState, templated
 * on the random stream, with the draw -> generator map).
 */
#ifndef PHT_HOST_LISTS_H
#define PHT_HOST_LISTS_H

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
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
  double bad_c = 0.0;                                /* its C */
  enum Bad { kOk = 0, kRange, kDiagonal, kAbsorbingRow, kCoefficient };
  Bad bad = kOk; /* why */

  /* 0, or -1 (bad_* say which cell, bad why) for a T[i,j] outside 0..m, a
   * non-zero T on the diagonal (a transient row's diagonal is minus the row's
   * sum, never a parameter) or in the absorbing row n (there is no z_n and no
   * N row n: the update would read past both), or a used cell whose C is not
   * finite and > 0 (z / C and theta C must be finite rates).  The reference
   * accepts all of these in its C code; its R wrappers refuse them */
  int build(int n, int m, const int *T, const double *C) {
    const int n1 = n + 1;
    for (auto *l : {&Nl, &Sl, &sl, &zl, &TTl}) l->assign(m, {});
    Dl.assign(n1, {});
    bad = kOk;
    for (int i = 0; i < n1; i++)
      for (int j = 0; j < n1; j++) {
        const int t = T[i + j * n1];
        if (t == 0) continue;
        const double c = C[i + j * n1];
        const Bad why = (t < 1 || t > m)                ? kRange
                        : (i == j)                      ? kDiagonal
                        : (i == n)                      ? kAbsorbingRow
                        : !(std::isfinite(c) && c > 0.0) ? kCoefficient
                                                         : kOk;
        if (why != kOk) {
          bad_i = i;
          bad_j = j;
          bad_t = t;
          bad_c = c;
          bad = why;
          return -1;
        }
        const int k = t - 1;
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

  /* the rejected cell and the reason, for the entry points' error text */
  void describe(char *buf, size_t len) const {
    switch (bad) {
      case kRange: std::snprintf(buf, len, "T[%d,%d] = %d outside 0..m", bad_i, bad_j, bad_t); break;
      case kDiagonal:
        std::snprintf(buf, len, "T[%d,%d] = %d is on the diagonal, which is minus the row's sum and holds no parameter",
                      bad_i, bad_j, bad_t);
        break;
      case kAbsorbingRow:
        std::snprintf(buf, len, "T[%d,%d] = %d is in the absorbing row, which has no rates", bad_i, bad_j, bad_t);
        break;
      case kCoefficient:
        std::snprintf(buf, len, "C[%d,%d] = %g of the cell T[%d,%d] = %d is not finite and > 0", bad_i, bad_j, bad_c,
                      bad_i, bad_j, bad_t);
        break;
      default: std::snprintf(buf, len, "no rejected cell"); break;
    }
  }
};

/* ============================================================ Gibbs core */
/* The map draw -> generator shared by GibbsState and pht_theta_to_S
 * (src/PHT_MCMC_Aslett.c:214-262, :380-397): cell (i, j) of the (n+1)^2
 * matrix TT with T[i + j n1] = k + 1 holds theta_k C[i + j n1]; the diagonal
 * of a transient row is minus the sum of the row's cells. */
inline double tt_cell(double theta, double c) { return theta * c; }
/* row i's diagonal.  reverse = false: cells by increasing column (how the
 * reference initialises the chain); true: by decreasing column, the
 * reverse-insertion order in which its update refreshes every later draw */
inline double tt_diag(int n1, const int *T, const double *TT, int i, bool reverse) {
  double tmp = 0.0;
  for (int q = 0; q < n1; q++) {
    const int j = reverse ? n1 - 1 - q : q;
    if (T[i + j * n1] != 0) tmp -= TT[i + j * n1];
  }
  return tmp;
}
/* (S, s) = the transient block and exit column of TT */
inline void tt_split(int n, const double *TT, double *S, double *s) {
  const int n1 = n + 1;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) S[i + j * n] = TT[i + j * n1];
  for (int i = 0; i < n; i++) s[i] = TT[i + n * n1];
}

/* The reference's Gibbs bookkeeping (src/PHT_MCMC_Aslett.c:187-405) with
 * the linked lists kept as arrays visited in list (reverse-insertion)
 * order, so zsum and the diagonal refresh sum in the reference's order. */
struct GibbsState {
  int it, n, m, n1;
  const double *nu, *zeta;
  const int *T;
  double *res;
  std::vector<double> TT, S, s;
  const std::vector<std::vector<Ent>> &Nl, &Sl, &sl, &zl, &TTl;

  /* L: the lists of (T, C), built by the caller (who reports a bad T) */
  template <class Rng>
  GibbsState(Rng &R, int it_, int n_, int m_, const double *nu_, const double *zeta_, const int *T_,
             const ParamLists &L, const double *start, double *res_)
      : it(it_), n(n_), m(m_), n1(n_ + 1), nu(nu_), zeta(zeta_), T(T_), res(res_),
        Nl(L.Nl), Sl(L.Sl), sl(L.sl), zl(L.zl), TTl(L.TTl) {
    TT.assign(n1 * n1, 0.0);
    S.assign(n * n, 0.0);
    s.assign(n, 0.0);
    if (start[0] < 0) {
      for (int i = 0; i < m; i++)
        res[0 + (size_t)i * it] = (nu[i] > 1) ? (nu[i] - 1.0) / zeta[i] : R.gamma(nu[i], 1.0 / zeta[i]);
    } else {
      for (int i = 0; i < m; i++) res[0 + (size_t)i * it] = start[i];
    }
    for (int k = 0; k < m; k++)
      for (const Ent &e : TTl[k]) TT[e.i + e.j * n1] = tt_cell(res[0 + (size_t)k * it], e.c);
    for (int i = 0; i < n1; i++) TT[i + i * n1] = tt_diag(n1, T, TT.data(), i, false);
    tt_split(n, TT.data(), S.data(), s.data());
  }

  /* steps 4-5 (:340-397): compile statistics and draw from the posteriors */
  template <class Rng>
  void update(Rng &R, int iter, const double *z, const long long *Nt) {
    std::vector<long long> Nsum(m, 0);
    std::vector<double> zsum(m, 0.0);
    for (int k = 0; k < m; k++) {
      for (int e = (int)Nl[k].size() - 1; e >= 0; e--) Nsum[k] += Nt[Nl[k][e].i + Nl[k][e].j * n];
      for (int e = (int)zl[k].size() - 1; e >= 0; e--) zsum[k] += z[zl[k][e].i] / zl[k][e].c;
    }
    for (int k = 0; k < m; k++) {
      const double tmp = res[iter + (size_t)k * it] =
          R.gamma(nu[k] + (double)(int)Nsum[k], 1.0 / (zeta[k] + zsum[k]));
      for (int e = (int)TTl[k].size() - 1; e >= 0; e--)
        TT[TTl[k][e].i + TTl[k][e].j * n1] = tt_cell(tmp, TTl[k][e].c);
      for (int e = (int)Sl[k].size() - 1; e >= 0; e--) S[Sl[k][e].i + Sl[k][e].j * n] = tt_cell(tmp, Sl[k][e].c);
      for (int e = (int)sl[k].size() - 1; e >= 0; e--) s[sl[k][e].i] = tt_cell(tmp, sl[k][e].c);
    }
    for (int i = 0; i < n; i++) { /* Dl[i] in reverse = the row's cells by decreasing column */
      const double tmp = tt_diag(n1, T, TT.data(), i, true);
      TT[i + i * n1] = tmp;
      S[i + i * n] = tmp;
    }
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
