/*
 * replace_draw_check.c — include/pht_replace.h's host function for one draw,
 * alone (tests/test_replace_host_check.py builds it with the address and
 * undefined-behaviour sanitizers where their runtime is there, and runs it; no
 * GPU, no Python in the process).  Every buffer has exactly the documented
 * size, so that an index past PHT_RP_WORK(G), the G curve words or the P policy
 * words is an error: n = 1, 3, 10 and 32; G = 1, 7 and 1024; P = 1, 2 and 16; a
 * last age at the table's cap (K = 1988), ages beyond the horizon, an unusable
 * cost pair, a flagged and a trapped draw.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pht_replace.h"

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      printf("FAILED %s (line %d)\n", #c, __LINE__);              \
      fails++;                                                    \
    }                                                             \
  } while (0)

/* a chain 0 -> 1 -> ... -> n-1 with rate lam, a fraction back to 0 and a fraction out of every state */
static void generator(int n, double lam, double *S, double *s) {
  memset(S, 0, sizeof(double) * (size_t)n * n);
  for (int i = 0; i < n; i++) {
    const double fwd = (i + 1 < n) ? 0.6 * lam : 0.0, back = (i > 0) ? 0.1 * lam : 0.0;
    s[i] = lam - fwd - back;
    S[i + i * n] = -lam;
    if (i + 1 < n) S[i + (i + 1) * n] = fwd;
    if (i > 0) S[i] = back; /* S[i][0], column-major */
  }
}

/* kind 0: usable; 1: a NaN in S; 2: a trap (state 0 never leaves) */
static void one(int n, int G, double first, double last, int P, int kind, unsigned want_flag, int want_beyond) {
  const double lam = 1.3;
  double *S = (double *)malloc(sizeof(double) * (size_t)n * n), *s = (double *)malloc(sizeof(double) * n);
  generator(n, lam, S, s);
  if (kind == 1) S[0] = NAN;
  if (kind == 2) {
    for (int j = 1; j < n; j++) S[j * n] = 0.0; /* row 0: no way out */
    s[0] = 0.0;
  }
  double *ages = (double *)malloc(sizeof(double) * G);
  for (int i = 0; i < G; i++) ages[i] = (G == 1) ? last : first + (last - first) * ((double)i / (double)(G - 1));
  double *cp = (double *)malloc(sizeof(double) * P), *cf = (double *)malloc(sizeof(double) * P);
  for (int p = 0; p < P; p++) {
    cp[p] = 1.0;
    cf[p] = 1.0 + 0.5 * (double)(p + 1) * (double)(p + 1);
  }
  if (P > 1) cf[1] = 0.5; /* cf < cp: unusable */
  double *work = (double *)malloc(sizeof(double) * PHT_RP_WORK(G));
  unsigned *af = (unsigned *)malloc(sizeof(unsigned) * G), *fl = (unsigned *)malloc(sizeof(unsigned) * P);
  double *lS = (double *)malloc(sizeof(double) * G), *lf = (double *)malloc(sizeof(double) * G);
  double *M = (double *)malloc(sizeof(double) * G);
  double *t = (double *)malloc(sizeof(double) * P), *g = (double *)malloc(sizeof(double) * P);
  double *lo = (double *)malloc(sizeof(double) * P), *hi = (double *)malloc(sizeof(double) * P);
  int *j = (int *)malloc(sizeof(int) * P), *nev = (int *)malloc(sizeof(int) * P);
  double m;
  CHECK(pht_rp_ages_ok(G, ages));
  const unsigned flag = pht_rp_draw(n, S, s, G, ages, P, cp, cf, work, af, lS, lf, M, &m, t, g, lo, hi, j, nev, fl);
  CHECK(flag == want_flag);
  int beyond = 0;
  for (int i = 0; i < G; i++) {
    if (flag) {
      CHECK(af[i] == PHT_RP_A_DRAW && M[i] != M[i]);
      continue;
    }
    beyond += (af[i] & PHT_RP_A_BEYOND) != 0;
    if (af[i])
      CHECK(lS[i] != lS[i] && lf[i] != lf[i] && M[i] != M[i]);
    else
      CHECK(M[i] > 0.0 && M[i] <= ages[i] * 1.0000001 && M[i] <= m * 1.0000001 && lS[i] <= 0.0);
  }
  CHECK(beyond == want_beyond);
  for (int p = 0; p < P; p++) {
    if (flag) {
      CHECK(fl[p] == PHT_RP_F_DRAW && t[p] != t[p] && j[p] == -1 && nev[p] == 0);
      continue;
    }
    if (!pht_rp_cost_ok(cp[p], cf[p])) {
      CHECK(fl[p] == PHT_RP_F_COST && t[p] != t[p] && g[p] != g[p]);
      continue;
    }
    CHECK(!(fl[p] & (PHT_RP_F_COST | PHT_RP_F_DRAW | PHT_RP_F_CAP)));
    if (fl[p] & (PHT_RP_F_NOAGE | PHT_RP_F_EVAL)) continue;
    CHECK(j[p] >= 0 && j[p] < G && lo[p] <= hi[p] && g[p] > 0.0 && g[p] <= cf[p] / m);
    if (fl[p] & PHT_RP_F_NEVER)
      CHECK(t[p] == INFINITY && g[p] == cf[p] / m);
    else
      CHECK(t[p] >= lo[p] && t[p] <= hi[p]);
    if (!(fl[p] & (PHT_RP_F_EDGE | PHT_RP_F_UNREFINED))) CHECK(nev[p] >= 1 && pht_rp_stop(lo[p], hi[p]));
  }
  free(S), free(s), free(ages), free(cp), free(cf), free(work), free(af), free(fl), free(lS), free(lf), free(M),
      free(t), free(g), free(lo), free(hi), free(j), free(nev);
}

int main(void) {
  one(1, 1, 0.0, 1.0, 1, 0, 0, 0);
  one(3, 7, 0.05, 3.2, 16, 0, 0, 0);
  one(10, 7, 0.1, 12.0, 2, 0, 0, 0);
  one(32, 1024, 0.01, 40.0, 16, 0, 0, 0);
  one(3, 1024, 0.5, 1400.0 / 1.3, 1, 0, 0, 0);  /* the last age at the cap: K = 1988 */
  one(32, 7, 100.0, 2800.0 / 1.3, 2, 0, 0, 4);  /* mu tau = 130, 575, 1020, 1465, ... 2800: four beyond */
  one(3, 7, 0.05, 3.2, 2, 1, PHT_LL_F_NONFINITE, 0);
  one(3, 7, 0.05, 3.2, 2, 2, PHT_CD_F_TRAP, 0);
  if (fails) return 1;
  printf("replace draw: ok\n");
  return 0;
}
