/*
 * Stand-alone check of phasetype_amd/csrc/host_lists.h (no HIP, no library):
 * the per-parameter lists of two structures against values written out by
 * hand from the walk (i outer, j inner; the reference's insertion order,
 * src/PHT_MCMC_Aslett.c:214-262), the rejection of a bad T, and the UNIF
 * table length; the refusals of build() (a cell on the diagonal, in the
 * absorbing row, a used cell whose C is not finite and > 0); and GibbsState
 * over its constructor and two updates on two tied, scaled structures, driven
 * by a recording random stream, against literals printed by
 * tests/update_cases.py (PYTHONPATH=. python tests/update_cases.py, from the
 * repository root).  Built and run by tests/test_host_lists.py, with the address
 * and undefined-behaviour sanitizers where the compiler has them.
 */
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <vector>

#include "host_lists.h"

using pht::host::Ent;
using pht::host::GibbsState;
using pht::host::ParamLists;
using pht::host::unif_rows;

static int g_bad = 0;
#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);  \
      g_bad++;                                                    \
    }                                                             \
  } while (0)

struct Cell {
  int i, j, t;
  double c;
};

/* column-major (n+1)^2 T and C from the non-zero cells */
static void fill(int n, std::initializer_list<Cell> cells, std::vector<int> &T, std::vector<double> &C) {
  const int n1 = n + 1;
  T.assign(n1 * n1, 0);
  C.assign(n1 * n1, 0.0);
  for (const Cell &c : cells) {
    T[c.i + c.j * n1] = c.t;
    C[c.i + c.j * n1] = c.c;
  }
}

static bool same(const std::vector<Ent> &got, std::initializer_list<Ent> want) {
  if (got.size() != want.size()) return false;
  size_t k = 0;
  for (const Ent &w : want) {
    if (got[k].i != w.i || got[k].j != w.j || got[k].c != w.c) return false;
    k++;
  }
  return true;
}

/* n = 2, m = 3: parameter 2 is the exit rate of both states */
static void two_states() {
  std::vector<int> T;
  std::vector<double> C;
  fill(2, {{0, 1, 1, 1.0}, {0, 2, 2, 0.5}, {1, 0, 3, 2.0}, {1, 2, 2, 1.5}}, T, C);
  ParamLists L;
  CHECK(L.build(2, 3, T.data(), C.data()) == 0);
  CHECK(L.Nl.size() == 3 && L.Sl.size() == 3 && L.sl.size() == 3 && L.zl.size() == 3 && L.TTl.size() == 3);
  CHECK(L.Dl.size() == 3);
  /* parameter 1: cell (0,1) */
  CHECK(same(L.Nl[0], {{0, 1, 1.0}}));
  CHECK(same(L.Sl[0], {{0, 1, 1.0}}));
  CHECK(same(L.sl[0], {}));
  CHECK(same(L.zl[0], {{0, 0, 1.0}}));
  CHECK(same(L.TTl[0], {{0, 1, 1.0}}));
  /* parameter 2: exit cells (0,2) then (1,2); N counts with the diagonal cell */
  CHECK(same(L.Nl[1], {{0, 0, 1.0}, {1, 1, 1.0}}));
  CHECK(same(L.Sl[1], {}));
  CHECK(same(L.sl[1], {{0, 0, 0.5}, {1, 0, 1.5}}));
  CHECK(same(L.zl[1], {{0, 0, 0.5}, {1, 0, 1.5}}));
  CHECK(same(L.TTl[1], {{0, 2, 0.5}, {1, 2, 1.5}}));
  /* parameter 3: cell (1,0) */
  CHECK(same(L.Nl[2], {{1, 0, 1.0}}));
  CHECK(same(L.Sl[2], {{1, 0, 2.0}}));
  CHECK(same(L.sl[2], {}));
  CHECK(same(L.zl[2], {{1, 0, 2.0}}));
  CHECK(same(L.TTl[2], {{1, 0, 2.0}}));
  /* rows: cells by increasing column */
  CHECK(same(L.Dl[0], {{0, 1, 1.0}, {0, 2, 1.0}}));
  CHECK(same(L.Dl[1], {{1, 0, 1.0}, {1, 2, 1.0}}));
  CHECK(same(L.Dl[2], {}));

  /* a T holding m + 1, or a negative entry, is rejected and named */
  T[1 + 2 * 3] = 4;
  CHECK(L.build(2, 3, T.data(), C.data()) == -1);
  CHECK(L.bad_i == 1 && L.bad_j == 2 && L.bad_t == 4);
  T[1 + 2 * 3] = 2;
  T[0 + 1 * 3] = -1;
  CHECK(L.build(2, 3, T.data(), C.data()) == -1);
  CHECK(L.bad_i == 0 && L.bad_j == 1 && L.bad_t == -1);
}

/* n = 3, m = 4: parameter 1 is cell (0,1) and state 3's exit rate,
 * parameter 2 state 1's exit rate and cell (1,2) */
static void three_states() {
  std::vector<int> T;
  std::vector<double> C;
  fill(3, {{0, 1, 1, 1.0}, {0, 3, 2, 2.0}, {1, 2, 2, 0.25}, {1, 3, 3, 1.0}, {2, 0, 4, 3.0}, {2, 3, 1, 0.5}}, T, C);
  ParamLists L;
  CHECK(L.build(3, 4, T.data(), C.data()) == 0);
  CHECK(same(L.Nl[0], {{0, 1, 1.0}, {2, 2, 1.0}}));
  CHECK(same(L.Sl[0], {{0, 1, 1.0}}));
  CHECK(same(L.sl[0], {{2, 0, 0.5}}));
  CHECK(same(L.zl[0], {{0, 0, 1.0}, {2, 0, 0.5}}));
  CHECK(same(L.TTl[0], {{0, 1, 1.0}, {2, 3, 0.5}}));
  CHECK(same(L.Nl[1], {{0, 0, 1.0}, {1, 2, 1.0}}));
  CHECK(same(L.Sl[1], {{1, 2, 0.25}}));
  CHECK(same(L.sl[1], {{0, 0, 2.0}}));
  CHECK(same(L.zl[1], {{0, 0, 2.0}, {1, 0, 0.25}}));
  CHECK(same(L.TTl[1], {{0, 3, 2.0}, {1, 2, 0.25}}));
  CHECK(same(L.Nl[2], {{1, 1, 1.0}}));
  CHECK(same(L.Sl[2], {}));
  CHECK(same(L.sl[2], {{1, 0, 1.0}}));
  CHECK(same(L.zl[2], {{1, 0, 1.0}}));
  CHECK(same(L.TTl[2], {{1, 3, 1.0}}));
  CHECK(same(L.Nl[3], {{2, 0, 1.0}}));
  CHECK(same(L.Sl[3], {{2, 0, 3.0}}));
  CHECK(same(L.sl[3], {}));
  CHECK(same(L.zl[3], {{2, 0, 3.0}}));
  CHECK(same(L.TTl[3], {{2, 0, 3.0}}));
  CHECK(same(L.Dl[0], {{0, 1, 1.0}, {0, 3, 1.0}}));
  CHECK(same(L.Dl[1], {{1, 2, 1.0}, {1, 3, 1.0}}));
  CHECK(same(L.Dl[2], {{2, 0, 1.0}, {2, 3, 1.0}}));
  CHECK(same(L.Dl[3], {}));
}

static void table_rows() {
  CHECK(unif_rows(0.0) == 64);
  /* 1449 + 14 sqrt(1449) + 64 = 2045.92..: the last length below the cap */
  CHECK(unif_rows(1449.0) == 2046);
  CHECK(unif_rows(1450.0) == 2047); /* 2047.10..: ceil is 2048, capped */
  CHECK(unif_rows(1e300) == 2047);
  CHECK(unif_rows(std::numeric_limits<double>::infinity()) == 2047);
  CHECK(unif_rows(std::nan("")) == 2047);
}

/* build() refuses what the update cannot index or scale */
static void refusals() {
  std::vector<int> T;
  std::vector<double> C;
  ParamLists L;
  char why[160];
  fill(2, {{0, 1, 1, 1.0}, {1, 2, 2, 1.0}, {1, 1, 1, 1.0}}, T, C); /* on the diagonal */
  CHECK(L.build(2, 2, T.data(), C.data()) == -1);
  CHECK(L.bad == ParamLists::kDiagonal && L.bad_i == 1 && L.bad_j == 1 && L.bad_t == 1);
  L.describe(why, sizeof why);
  CHECK(std::strstr(why, "T[1,1]") && std::strstr(why, "diagonal"));
  fill(2, {{0, 1, 1, 1.0}, {1, 2, 2, 1.0}, {2, 0, 2, 1.0}}, T, C); /* in row n */
  CHECK(L.build(2, 2, T.data(), C.data()) == -1);
  CHECK(L.bad == ParamLists::kAbsorbingRow && L.bad_i == 2 && L.bad_j == 0 && L.bad_t == 2);
  L.describe(why, sizeof why);
  CHECK(std::strstr(why, "T[2,0]") && std::strstr(why, "absorbing row"));
  fill(2, {{0, 1, 1, 1.0}, {1, 2, 2, 1.0}, {2, 2, 2, 1.0}}, T, C); /* the corner: on the diagonal of row n */
  CHECK(L.build(2, 2, T.data(), C.data()) == -1 && L.bad_i == 2 && L.bad_j == 2);
  const double inf = std::numeric_limits<double>::infinity();
  for (double c : {0.0, -1.0, inf, std::nan("")}) {
    fill(2, {{0, 1, 1, 1.0}, {1, 2, 2, c}}, T, C);
    CHECK(L.build(2, 2, T.data(), C.data()) == -1);
    CHECK(L.bad == ParamLists::kCoefficient && L.bad_i == 1 && L.bad_j == 2 && L.bad_t == 2);
    L.describe(why, sizeof why);
    CHECK(std::strstr(why, "C[1,2]") && std::strstr(why, "not finite and > 0"));
  }
  /* the C of an unused cell is not looked at, and a good build clears the reason */
  fill(2, {{0, 1, 1, 1.0}, {1, 2, 2, 1.0}}, T, C);
  C[1 + 0 * 3] = 0.0;
  C[2 + 2 * 3] = std::nan("");
  CHECK(L.build(2, 2, T.data(), C.data()) == 0 && L.bad == ParamLists::kOk);
}

/* the random stream of a GibbsState run: preset draws, every call logged */
struct RecRng {
  std::vector<double> preset, log; /* log: shape, scale per call */
  size_t at = 0;
  double gamma(double a, double scale) {
    log.push_back(a);
    log.push_back(scale);
    return at < preset.size() ? preset[at++] : std::nan("");
  }
};

static bool same_bits(const double *got, const double *want, size_t len) {
  return std::memcmp(got, want, len * sizeof(double)) == 0;
}

/* S and s are the transient block and the exit column of want (TT) */
static bool split_of(const GibbsState &G, const double *want) {
  const int n = G.n, n1 = n + 1;
  for (int i = 0; i < n; i++) {
    for (int j = 0; j < n; j++)
      if (std::memcmp(&G.S[i + j * n], &want[i + j * n1], sizeof(double)) != 0) return false;
    if (std::memcmp(&G.s[i], &want[i + n * n1], sizeof(double)) != 0) return false;
  }
  return true;
}

/* one run: the constructor, then two updates from hand-written z (fixed point
 * zq 2^-zexp) and N (column-major N[i + j n], exit counts on the diagonal) */
static void gibbs_run(int n, int m, std::initializer_list<Cell> cells, const double *nu, const double *zeta,
                      const double *start, std::initializer_list<double> preset, int zexp, const long long (*zq)[3],
                      const long long (*N)[9], int ctor_draws, const double *TT0, const double *const *args,
                      const double *const *TTu) {
  std::vector<int> T;
  std::vector<double> C;
  fill(n, cells, T, C);
  ParamLists L;
  CHECK(L.build(n, m, T.data(), C.data()) == 0);
  RecRng R;
  R.preset = preset;
  const int it = 3;
  std::vector<double> res((size_t)it * m, 0.0);
  GibbsState G(R, it, n, m, nu, zeta, T.data(), L, start, res.data());
  CHECK((int)R.log.size() == 2 * ctor_draws);
  CHECK(same_bits(G.TT.data(), TT0, (size_t)(n + 1) * (n + 1)));
  CHECK(split_of(G, TT0));
  for (int u = 1; u <= 2; u++) {
    double z[3];
    for (int i = 0; i < n; i++) z[i] = std::ldexp((double)zq[u - 1][i], -zexp);
    R.log.clear();
    G.update(R, u, z, N[u - 1]);
    CHECK((int)R.log.size() == 2 * m);
    for (int k = 0; k < m; k++) { /* args: shape, scale per parameter */
      CHECK(same_bits(&R.log[2 * k], &args[u - 1][2 * k], 1));
      CHECK(same_bits(&R.log[2 * k + 1], &args[u - 1][2 * k + 1], 1));
      CHECK(res[u + (size_t)k * it] == R.preset[ctor_draws + (u - 1) * m + k]);
    }
    CHECK(same_bits(G.TT.data(), TTu[u - 1], (size_t)(n + 1) * (n + 1)));
    CHECK(split_of(G, TTu[u - 1]));
  }
}

static void gibbs_state() {
  /* fr3c: constructor */
  static const double fr3c_TT0[] = {-0x1.5000000000000p+2, 0x1.6800000000000p+3, 0x1.0e00000000000p+3, 0x0.0p+0, 0x1.8000000000000p+0, -0x1.b4ccccccccccdp+3, 0x0.0p+0, 0x0.0p+0, 0x1.e000000000000p+1, 0x0.0p+0, -0x1.3e00000000000p+3, 0x0.0p+0, 0x0.0p+0, 0x1.3333333333334p+1, 0x1.8000000000000p+0, 0x0.0p+0};
  /* fr3c: update 1 */
  static const double fr3c_args1[] = {0x1.8000000000000p+5, 0x1.a441b90b39426p-5, 0x1.7a00000000000p+7, 0x1.9b2c34e2b7980p-5};
  static const double fr3c_TT1[] = {-0x1.3400000000000p+2, 0x1.5000000000000p+3, 0x1.f800000000000p+2, 0x0.0p+0, 0x1.6000000000000p+0, -0x1.9666666666666p+3, 0x0.0p+0, 0x0.0p+0, 0x1.b800000000000p+1, 0x0.0p+0, -0x1.2800000000000p+3, 0x0.0p+0, 0x0.0p+0, 0x1.199999999999ap+1, 0x1.6000000000000p+0, 0x0.0p+0};
  /* fr3c: update 2 */
  static const double fr3c_args2[] = {0x1.8800000000000p+5, 0x1.c6becfa5114d1p-5, 0x1.8400000000000p+7, 0x1.c1f9ee2cf58cdp-5};
  static const double fr3c_TT2[] = {-0x1.6c00000000000p+2, 0x1.8800000000000p+3, 0x1.2600000000000p+3, 0x0.0p+0, 0x1.a000000000000p+0, -0x1.db33333333333p+3, 0x0.0p+0, 0x0.0p+0, 0x1.0400000000000p+2, 0x0.0p+0, -0x1.5a00000000000p+3, 0x0.0p+0, 0x0.0p+0, 0x1.4cccccccccccdp+1, 0x1.a000000000000p+0, 0x0.0p+0};
  /* tri3: constructor */
  static const double tri3_TT0[] = {-0x1.0000000000000p+51, 0x0.0p+0, 0x1.cccccccccccccp-1, 0x0.0p+0, 0x1.0000000000000p+51, -0x1.3333333333333p-3, 0x0.0p+0, 0x0.0p+0, 0x1.0000000000000p-2, 0x0.0p+0, -0x1.4666666666666p+0, 0x0.0p+0, 0x1.0000000000000p-2, 0x1.3333333333333p-3, 0x1.8000000000000p-2, 0x0.0p+0};
  /* tri3: update 1 */
  static const double tri3_args1[] = {0x1.8000000000000p+3, 0x1.9b72c3fafa396p-3, 0x1.3b33333333333p+4, 0x1.6c68465ad4fbap-3};
  static const double tri3_TT1[] = {-0x1.8000000000002p+52, 0x0.0p+0, 0x1.4666666666666p+2, 0x0.0p+0, 0x1.8000000000000p+52, -0x1.b333333333333p-1, 0x0.0p+0, 0x0.0p+0, 0x1.8000000000000p-1, 0x0.0p+0, -0x1.ce66666666666p+2, 0x0.0p+0, 0x1.8000000000000p-1, 0x1.b333333333333p-1, 0x1.1000000000000p+1, 0x0.0p+0};
  /* tri3: update 2 */
  static const double tri3_args2[] = {0x1.2000000000000p+4, 0x1.ffd0047f940a2p-4, 0x1.8b33333333333p+4, 0x1.0eeb66aa045a2p-2};
  static const double tri3_TT2[] = {-0x1.0000000000001p+53, 0x0.0p+0, 0x1.599999999999ap+1, 0x0.0p+0, 0x1.0000000000000p+53, -0x1.ccccccccccccdp-2, 0x0.0p+0, 0x0.0p+0, 0x1.0000000000000p+0, 0x0.0p+0, -0x1.e99999999999ap+1, 0x0.0p+0, 0x1.0000000000000p+0, 0x1.ccccccccccccdp-2, 0x1.2000000000000p+0, 0x0.0p+0};

  { /* fr3c (tests/update_cases.py): F in four cells, R in two, three multipliers off 1; a given start */
    const double nu[] = {24.0, 180.0}, zeta[] = {16.0, 16.0}, start[] = {1.5, 11.25};
    const long long zq[2][3] = {{517, 1283, 2051}, {333, 777, 1111}};
    const long long N[2][9] = {{0, 6, 3, 7, 4, 0, 5, 0, 8}, {0, 1, 13, 2, 11, 0, 9, 0, 3}};
    const double *args[] = {fr3c_args1, fr3c_args2}, *TTu[] = {fr3c_TT1, fr3c_TT2};
    gibbs_run(3, 2, {{0, 1, 1, 1.0}, {0, 2, 1, 2.5}, {1, 3, 1, 1.6}, {2, 3, 1, 1.0}, {1, 0, 2, 1.0}, {2, 0, 2, 0.75}}, nu,
              zeta, start, {1.375, 10.5, 1.625, 12.25}, 10, zq, N, 0, fr3c_TT0, args, TTu);
  }
  { /* tri3: three cells per parameter; row 0 = (2^53, 1, 1) theta sums to another value by increasing column
     * (the constructor) than by decreasing column (every update); parameter 2 starts from a prior draw */
    const double nu[] = {2.0, 0.7}, zeta[] = {4.0, 2.0}, start[] = {-1.0};
    const long long zq[2][3] = {{1001, 2003, 3007}, {4099, 123, 2999}};
    const long long N[2][9] = {{5, 0, 4, 3, 9, 0, 2, 0, 6}, {1, 0, 10, 8, 2, 0, 7, 0, 12}};
    const double *args[] = {tri3_args1, tri3_args2}, *TTu[] = {tri3_TT1, tri3_TT2};
    gibbs_run(3, 2, {{0, 1, 1, 0x1p53}, {0, 2, 1, 1.0}, {0, 3, 1, 1.0}, {1, 3, 2, 0.5}, {2, 0, 2, 3.0}, {2, 3, 2, 1.25}},
              nu, zeta, start, {0.3, 0.75, 1.7, 1.0, 0.9}, 11, zq, N, 1, tri3_TT0, args, TTu);
    /* the two orders: 0.25 (2^53 + 1 + 1) forward loses both ones, backward keeps them */
    const double th = 0.25, big = th * 0x1p53;
    CHECK(((0.0 - big) - th) - th != ((0.0 - th) - th) - big);
    CHECK(tri3_TT0[0] == ((0.0 - big) - th) - th);
  }
}

int main() {
  two_states();
  three_states();
  refusals();
  gibbs_state();
  table_rows();
  if (g_bad) return 1;
  std::printf("host lists: ok\n");
  return 0;
}
