/*
 * oracle/ref_entry.c — TEST INFRASTRUCTURE ONLY.
 *
 * Entry points into the reference's own compiled C (oracle/_ref/libpht_ref.so,
 * built by oracle/Makefile's ref target from the reference's sources where
 * they lie, on the R-API stand-in of oracle/rshim/).  The reference's
 * declarations come from its own headers, found through -I: none is restated
 * here.
 *
 *   ref_gibbs  LJMA_Gibbs with its 15 .C vectors, as R's .C would call it.
 *   ref_eigen  LJMA_LAPACKspace + LJMA_eigen.
 *   ref_sweep  one step 1 at a fixed (S, s), one call of the reference's
 *              LJMA_MHsample_* per observation: B, z, N and the MT words
 *              that observation drew.  The samplers keep nothing from one
 *              observation to the next but the RNG stream, so the draws are
 *              those of one call over all observations.
 *
 * What ref_sweep prepares for the samplers (the jump-chain matrices and the
 * spectral products) is computed here; the chain's own preparation is the
 * reference's and is exercised through ref_gibbs.
 */
#include <stdint.h>

#include "R.h"
#include "R_ext/BLAS.h"

#include "PHT_MCMC_Aslett.h"
#include "utility.h"
#include "Simulate_AbsCTMC_eq_Bladt_MHRS.h"
#include "Simulate_AbsCTMC_eq_Aslett_ECS.h"
#include "Simulate_AbsCTMC_eq_AslettHobolth_DCS.h"

void rshim_free_all(void);
unsigned long long rshim_nword(void);

#define REF_WORK 100000 /* the chain's workspace size, doubles and ints */

void ref_gibbs(int *it, int *mhit, int *method, int *n, int *m, double *nu, double *zeta, int *T, double *C,
               double *y, int *l, int *censored, double *start, int *silent, double *res) {
  LJMA_Gibbs(it, mhit, method, n, m, nu, zeta, T, C, y, l, censored, start, silent, res);
  rshim_free_all();
}

/* S, Q, Qinv column-major n x n; returns LJMA_eigen's status */
int ref_eigen(int n, const double *S, double *evals, double *Q, double *Qinv) {
  int nn = n;
  double *workD = (double *)calloc(REF_WORK, sizeof(double));
  int *workI = (int *)calloc(REF_WORK, sizeof(int));
  LJMA_LAPACKspace(&nn);
  int info = LJMA_eigen(&nn, (double *)S, evals, Q, Qinv, workD, workI);
  LJMA_LAPACKspaceFree();
  free(workD);
  free(workI);
  rshim_free_all();
  return info;
}

/* Row i of the two jump-chain matrices of (S, s): over the transient states
 * (P) and with the exit as column n (Pfull).  The ratios to the diagonal are
 * summed left to right, the exit ratio after them and the diagonal's own
 * ratio taken off last, and each ratio is divided by its row's sum. */
static void jump_row(int n, int i, const double *S, const double *s, double *P, double *Pfull) {
  const double d = S[i + i * n];
  double acc = 0.0;
  for (int j = 0; j < n; j++) {
    const double q = -S[i + j * n] / d;
    P[i + j * n] = q;
    Pfull[i + j * n] = q;
    acc += q;
  }
  const double own = P[i + i * n];
  const double inner = acc - own;
  const double ex = -s[i] / d;
  double full = acc + ex;
  full -= own;
  P[i + i * n] = 0.0;
  Pfull[i + i * n] = 0.0;
  for (int j = 0; j < n; j++) {
    P[i + j * n] = P[i + j * n] / inner;
    Pfull[i + j * n] = Pfull[i + j * n] / full;
  }
  Pfull[i + n * n] = ex / full;
}

/*
 * method: the chain's bit mask, resolved in the chain's order (MHRS, then
 * DCS, then ECS).  Outputs per observation c: B[c] the starting state, z[c n
 * + k], N[c n n + i + j n] (column-major, exits on the diagonal), nd[c] the
 * 32-bit MT words drawn.  Returns LJMA_eigen's status (0 for MHRS), or -1
 * for a mask without a sampler bit.
 */
int ref_sweep(int method, int n, const double *S, const double *s, int mhit, const double *y, const int *censored,
              int l, double *z, int *B, int *N, unsigned *nd) {
  if (!(method & 0x7)) return -1;
  const size_t nn2 = (size_t)n * n;
  double *P = (double *)calloc(nn2, sizeof(double)), *Pfull = (double *)calloc(nn2 + n, sizeof(double));
  double *Q = (double *)calloc(nn2, sizeof(double)), *Qinv = (double *)calloc(nn2, sizeof(double));
  double *vec = (double *)calloc(8 * (size_t)n, sizeof(double));
  double *evals = vec, *ones = vec + n, *Qinv_s = vec + 2 * n, *Qinv_1 = vec + 3 * n, *Qinv_b = vec + 4 * n,
         *b = vec + 5 * n, *pi = vec + 6 * n, *sc = vec + 7 * n;
  double *Sc = (double *)malloc(nn2 * sizeof(double));
  double *workD = (double *)calloc(REF_WORK, sizeof(double)), *rz = (double *)calloc(n, sizeof(double));
  int *workI = (int *)calloc(REF_WORK, sizeof(int)), *rB = (int *)calloc(n, sizeof(int)),
      *rN = (int *)calloc(nn2, sizeof(int));
  memcpy(Sc, S, nn2 * sizeof(double));
  memcpy(sc, s, n * sizeof(double));
  pi[0] = 1.0;
  for (int i = 0; i < n; i++) {
    ones[i] = 1.0;
    b[i] = sc[i] > 0.0 ? 1.0 : 0.0;
    jump_row(n, i, Sc, sc, P, Pfull);
  }
  int nI = n, one = 1, mh = mhit, info = 0;
  double oneD = 1.0, zeroD = 0.0;
  char tN = 'N';
  const int which = (method & 0x1) ? 1 : (method & 0x4) ? 4 : 2;
  if (which != 1) {
    LJMA_LAPACKspace(&nI);
    info = LJMA_eigen(&nI, Sc, evals, Q, Qinv, workD, workI);
    LJMA_LAPACKspaceFree();
    if (which == 4) {
      F77_CALL(dgemv)(&tN, &nI, &nI, &oneD, Qinv, &nI, b, &one, &zeroD, Qinv_b, &one FCONE);
    } else {
      F77_CALL(dgemv)(&tN, &nI, &nI, &oneD, Qinv, &nI, sc, &one, &zeroD, Qinv_s, &one FCONE);
      F77_CALL(dgemv)(&tN, &nI, &nI, &oneD, Qinv, &nI, ones, &one, &zeroD, Qinv_1, &one FCONE);
    }
  }
  for (int c = 0; c < l; c++) {
    int m1 = 1;
    double *yp = (double *)y + c;
    int *cp = (int *)censored + c;
    const unsigned long long w0 = rshim_nword();
    if (which == 1)
      LJMA_MHsample_Bladt(yp, cp, &m1, pi, Sc, sc, Pfull, &nI, &mh, rz, rB, rN, workD, workI);
    else if (which == 4)
      LJMA_MHsample_Hobolth2(yp, cp, &m1, pi, Sc, sc, Q, evals, Qinv_b, b, Qinv, &nI, &mh, rz, rB, rN, workD,
                             workI);
    else
      LJMA_MHsample_Aslett2(yp, cp, &m1, pi, Sc, sc, Q, evals, Qinv_s, Qinv_1, P, Pfull, &nI, rz, rB, rN, workD,
                            workI);
    nd[c] = (unsigned)(rshim_nword() - w0);
    int first = 0;
    for (int k = 0; k < n; k++)
      if (rB[k]) first = k;
    B[c] = first;
    memcpy(z + (size_t)c * n, rz, n * sizeof(double));
    memcpy(N + (size_t)c * nn2, rN, nn2 * sizeof(int));
  }
  free(P); free(Pfull); free(Q); free(Qinv); free(vec); free(Sc); free(workD); free(rz); free(workI); free(rB);
  free(rN);
  rshim_free_all();
  return info;
}
