/*
 * spares_draw_check.c — include/pht_spares.h's host function for one draw,
 * alone (tests/test_spares_host_check.py builds it with the address and
 * undefined-behaviour sanitizers where their runtime is there, and runs it; no
 * GPU, no Python in the process).  Every buffer has exactly the documented
 * size, so that an index past PHT_SP_WORK, the words or the per-unit sums is an
 * error: n = 1, 3, 10 and 32, nh = 1 and 16, h = 0, a horizon just below the
 * renewal table's cap (Kr about 2036), a unit beyond the table, a flagged
 * draw.  r_h must be pht_cd_renewal's bit for bit.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pht_spares.h"

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

static void one(int n, int nh, const double *h, double lam, unsigned want_flag) {
  const long nc = 7;
  double *S = (double *)malloc(sizeof(double) * (size_t)n * n), *s = (double *)malloc(sizeof(double) * n);
  generator(n, lam, S, s);
  double c[7] = {0.0, 1e-6, 0.3, 1.0, 4.0, 9.0, 3000.0 / lam}; /* the last lies beyond every table */
  double *work = (double *)malloc(sizeof(double) * PHT_SP_WORK(n, nh));
  long long *words = (long long *)malloc(sizeof(long long) * pht_sp_nwords(nh)), *cnt = (long long *)calloc(nc, 8);
  double *scales = (double *)malloc(sizeof(double) * 2 * nh);
  double *dsum = (double *)calloc((size_t)nc * nh, 8), *vsum = (double *)calloc((size_t)nc * nh, 8);
  double *d2sum = (double *)calloc((size_t)nc * nh, 8);
  double *dd = (double *)malloc(sizeof(double) * nc * nh), *var = (double *)malloc(sizeof(double) * nc * nh);
  unsigned flag = 0;
  for (int rep = 0; rep < 2; rep++) /* two draws: the sums continue */
    flag = pht_sp_draw(n, S, s, nc, c, 9.0, nh, h, work, words, scales, dsum, vsum, d2sum, cnt, dd, var);
  CHECK(flag == want_flag);
  if (!flag) {
    CHECK(words[pht_sp_w_nbad(nh)] == 1 && words[pht_sp_w_nunits(nh)] == nc - 1);
    for (long i = 0; i < nc; i++) {
      CHECK(cnt[i] == ((i == nc - 1) ? 0 : 2));
      for (int j = 0; j < nh; j++) {
        const double v = var[i * nh + j], d = dd[i * nh + j];
        if (i == nc - 1) {
          CHECK(v != v && d != d);
          continue;
        }
        CHECK(v >= 0.0 && d >= 0.0 && v <= scales[nh + j] * 1.0000001 && d <= scales[j] * 1.0000001);
        CHECK(dsum[i * nh + j] == d + d && vsum[i * nh + j] == v + v);
        if (h[j] == 0.0) CHECK(v == 0.0 && d == 0.0);
      }
    }
    /* r_h against pht_cd_renewal, bit for bit */
    const double mu = lam;
    const int Kr = pht_llu_K(mu, h[nh - 1]);
    double *W = (double *)malloc(sizeof(double) * PHT_SP_WDOUBLES(nh, Kr + 1));
    double *T = (double *)malloc(sizeof(double) * (size_t)nh * (Kr + 1));
    double *r = (double *)malloc(sizeof(double) * nh * n), *q = (double *)malloc(sizeof(double) * nh * n);
    double *rc = (double *)malloc(sizeof(double) * nh * n), *sc = (double *)malloc(sizeof(double) * 2 * nh);
    pht_sp_vectors(n, S, s, mu, nh, h, W, r, q, sc);
    CHECK(pht_cd_renewal(n, S, s, mu, nh, h, T, rc) == 0);
    CHECK(memcmp(r, rc, sizeof(double) * nh * n) == 0 && memcmp(sc, scales, sizeof(double) * 2 * nh) == 0);
    free(W), free(T), free(r), free(q), free(rc), free(sc);
  } else {
    for (int j = 0; j < pht_sp_nwords(nh); j++) CHECK(words[j] == 0);
    for (long i = 0; i < nc; i++) CHECK(cnt[i] == 0 && var[i * nh] != var[i * nh]);
  }
  free(S), free(s), free(work), free(words), free(cnt), free(scales), free(dsum), free(vsum), free(d2sum), free(dd),
      free(var);
}

int main(void) {
  double h16[16] = {0.0, 1e-9};
  for (int j = 2; j < 16; j++) h16[j] = 0.001 * (double)(1 << (j - 2));
  const double h1[1] = {0.7}, hcap[2] = {1.0, 1440.0 / 1.3}, hover[2] = {1.0, 1600.0 / 1.3};
  one(1, 1, h1, 1.3, 0);
  one(3, 16, h16, 1.3, 0);
  one(10, 16, h16, 1.3, 0);
  one(32, 16, h16, 1.3, 0);
  one(3, 2, hcap, 1.3, 0);
  one(32, 2, hcap, 1.3, 0);
  one(3, 2, hover, 1.3, PHT_CD_F_HCAP);
  if (fails) return 1;
  printf("spares draw: ok\n");
  return 0;
}
