/*
 * replace_spec.c — CPU restatement of include/pht_replace.h over plain
 * arrays: the bit-level checker of the replacement kernels
 * (tests/replace_ref.py compiles it with -ffp-contract=off into a shared
 * object; no main).  The draw's meta words, table and evaluator are
 * include/pht_loglik_unif.h's, the mean include/pht_condition.h's.
 */
#include <stdlib.h>

#include "pht_replace.h"

double rpspec_rtol(void) { return PHT_RP_RTOL; }
int rpspec_maxstep(void) { return PHT_RP_MAXSTEP; }
double rpspec_M_R(void) { return PHT_RP_M_R; }
double rpspec_D_R(void) { return PHT_RP_D_R; }
size_t rpspec_work(int G) { return PHT_RP_WORK(G); }
int rpspec_ages_ok(int G, const double *ages) { return pht_rp_ages_ok(G, ages); }
double rpspec_eps(int n, int khi) { return pht_rp_eps(n, khi); }
double rpspec_M_bound(int n, int khi, double M) { return pht_rp_M_bound(n, khi, M); }
double rpspec_D_bound(int n, int khi, double hM, double F, double c0) { return pht_rp_D_bound(n, khi, hM, F, c0); }
double rpspec_g(double lS, double M, double cp, double cf) { return pht_rp_g(lS, M, cp, cf); }
double rpspec_D(double lS, double lf, double M, double cp, double cf) {
  return pht_rp_D(lS, lf, M, pht_rp_c0(cp, cf));
}

/* the draw's meta words [flag, mu, abar_x, K], its horizon and m */
unsigned rpspec_meta(int n, const double *S, const double *s, double tmax, double *meta, double *thi, double *m) {
  return pht_rp_meta(n, S, s, tmax, meta, thi, m);
}

/* (lS, lf, M, the largest window end, bad) at nt times of a usable draw whose
 * table is sized for tmax; returns the draw's flag word */
unsigned rpspec_eval(int n, const double *S, const double *s, double tmax, int nt, const double *t, double *lS,
                     double *lf, double *M, int *khi, int *bad) {
  double meta[PHT_LLU_META], thi, m;
  const unsigned flag = pht_rp_meta(n, S, s, tmax, meta, &thi, &m);
  if (flag) return flag;
  const int rows = PHT_LLU_MAXK + 1, K = (int)meta[PHT_LLU_M_K];
  double *tab = (double *)malloc(sizeof(double) * 4 * rows), *cc = tab + 2 * rows, *invk = tab + 3 * rows;
  pht_llu_table(n, S, s, meta[PHT_LLU_M_MU], K, tab);
  pht_rp_cc(tab, K, cc);
  for (int k = 0; k <= K; k++) invk[k] = k ? 1.0 / (double)k : 0.0;
  for (int i = 0; i < nt; i++)
    bad[i] = pht_rp_eval3(tab, cc, invk, K, meta[PHT_LLU_M_MU], meta[PHT_LLU_M_ABAR], t[i], &lS[i], &lf[i], &M[i],
                          &khi[i]);
  free(tab);
  return 0u;
}

/* pht_rp_rmean alone (M, its window end, bad) at nt times, the table sized for tmax */
unsigned rpspec_rmean(int n, const double *S, const double *s, double tmax, int nt, const double *t, double *M,
                      int *khi, int *bad) {
  double meta[PHT_LLU_META], thi, m;
  const unsigned flag = pht_rp_meta(n, S, s, tmax, meta, &thi, &m);
  if (flag) return flag;
  const int rows = PHT_LLU_MAXK + 1, K = (int)meta[PHT_LLU_M_K];
  double *tab = (double *)malloc(sizeof(double) * 4 * rows), *cc = tab + 2 * rows, *invk = tab + 3 * rows;
  pht_llu_table(n, S, s, meta[PHT_LLU_M_MU], K, tab);
  pht_rp_cc(tab, K, cc);
  for (int k = 0; k <= K; k++) invk[k] = k ? 1.0 / (double)k : 0.0;
  for (int i = 0; i < nt; i++) M[i] = pht_rp_rmean(cc, invk, K, meta[PHT_LLU_M_MU], t[i], &bad[i], &khi[i]);
  free(tab);
  return 0u;
}

/* pht_rp_policy of a usable draw at unit level: the curve from the draw's own
 * table (K rows for the last age), the policy then run on the first
 * min(K, Kuse) rows only.  Kuse >= K is pht_rp_draw's policy; a short Kuse
 * makes the points inside the bracket bad (the upward sweep ends at the
 * table's end) while the bracket's ends stay the curve's good ages: the
 * PHT_RP_F_EVAL path.  out7: t, g, lo, hi; outi: j, nev, flags. */
unsigned rpspec_policy_K(int n, const double *S, const double *s, int G, const double *ages, double cp, double cf,
                         int Kuse, double *out4, int *outi) {
  double *work = (double *)malloc(sizeof(double) * PHT_RP_WORK(G));
  unsigned *af = (unsigned *)malloc(sizeof(unsigned) * (size_t)G);
  const int rows = PHT_LLU_MAXK + 1;
  double meta[PHT_LLU_META], thi, m, t, g, lo, hi;
  int j, nev;
  unsigned fl;
  const unsigned flag = pht_rp_draw(n, S, s, G, ages, 1, &cp, &cf, work, af, NULL, NULL, NULL, &m, &t, &g, &lo, &hi, &j,
                                    &nev, &fl);
  if (!flag) {
    pht_rp_meta(n, S, s, ages[G - 1], meta, &thi, &m);
    const int K = (int)meta[PHT_LLU_M_K], Kp = (Kuse < K) ? Kuse : K;
    double *tab = work, *cc = work + 2 * rows, *invk = work + 3 * rows, *lS = work + 4 * rows;
    pht_rp_out_t o;
    pht_rp_policy(tab, cc, invk, Kp, meta[PHT_LLU_M_MU], meta[PHT_LLU_M_ABAR], m, G, ages, lS, lS + G, lS + 2 * G, af,
                  cp, cf, &o);
    out4[0] = o.t, out4[1] = o.g, out4[2] = o.lo, out4[3] = o.hi;
    outi[0] = o.j, outi[1] = o.nev, outi[2] = (int)o.flags;
  }
  free(work);
  free(af);
  return flag;
}

/* the curve and P policies of one draw; returns the draw's flag word */
unsigned rpspec_draw(int n, const double *S, const double *s, int G, const double *ages, int P, const double *cp,
                     const double *cf, unsigned *aflags, double *lS, double *lf, double *M, double *m, double *t,
                     double *g, double *lo, double *hi, int *j, int *nev, unsigned *flags) {
  double *work = (double *)malloc(sizeof(double) * PHT_RP_WORK(G));
  const unsigned flag = pht_rp_draw(n, S, s, G, ages, P, cp, cf, work, aflags, lS, lf, M, m, t, g, lo, hi, j, nev,
                                    flags);
  free(work);
  return flag;
}
