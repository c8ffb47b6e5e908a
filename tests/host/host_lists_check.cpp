/*
 * Stand-alone check of phasetype_amd/csrc/host_lists.h (no HIP, no library):
 * the per-parameter lists of two structures against values written out by
 * hand from the walk (i outer, j inner; the reference's insertion order,
 * src/PHT_MCMC_Aslett.c:214-262), the rejection of a bad T, and the UNIF
 * table length.  Built and run by tests/test_host_lists.py, with the address
 * and undefined-behaviour sanitizers where the compiler has them.
 */
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <limits>
#include <vector>

#include "host_lists.h"

using pht::host::Ent;
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

int main() {
  two_states();
  three_states();
  table_rows();
  if (g_bad) return 1;
  std::printf("host lists: ok\n");
  return 0;
}
