/*
 * host_params.cpp — the packed per-sweep parameter block (pht_layout.h) and
 * what it needs: the LAPACK binding, the reference's eigensystem call and the
 * device-mode spectral products.
 */
#include <dlfcn.h>
#include <math.h>
#include <string.h>

#include "host_internal.h"
#include "pht_detmath.h"

using namespace pht;
using namespace pht::host;

/* ================================================================ LAPACK */
namespace {
typedef void (*dgeevx_t)(const char *, const char *, const char *, const char *, const int *, double *,
                         const int *, double *, double *, double *, const int *, double *, const int *, int *,
                         int *, double *, double *, double *, double *, double *, const int *, int *, int *,
                         size_t, size_t, size_t, size_t);
typedef void (*dgetrf_t)(const int *, const int *, double *, const int *, int *, int *);
typedef void (*dgetri_t)(const int *, double *, const int *, const int *, double *, const int *, int *);
dgeevx_t p_dgeevx = nullptr;
dgetrf_t p_dgetrf = nullptr;
dgetri_t p_dgetri = nullptr;
/* OpenBLAS's thread-count setter, when the bound LAPACK is OpenBLAS (returns
 * the previous count).  The per-sweep eigensystem is an n <= 20 problem: its
 * BLAS calls gain nothing from the thread pool and pay its hand-offs (n = 10:
 * 81 us per parameter block with the pool, 17 us on the calling thread; the
 * same bytes, tests/test_host.py) */
typedef int (*blas_threads_t)(int);
blas_threads_t p_blas_threads = nullptr;

/* the three routines (names with the library's prefix) from handle h */
bool lookup_lapack(void *h, const std::string &pre = "") {
  p_dgeevx = (dgeevx_t)dlsym(h, (pre + "dgeevx_").c_str());
  p_dgetrf = (dgetrf_t)dlsym(h, (pre + "dgetrf_").c_str());
  p_dgetri = (dgetri_t)dlsym(h, (pre + "dgetri_").c_str());
  p_blas_threads = (blas_threads_t)dlsym(h, "openblas_set_num_threads_local");
  if (p_dgeevx && p_dgetrf && p_dgetri) return true;
  p_dgeevx = nullptr;
  return false;
}
}  // namespace

bool pht::host::lapack_ready() {
  if (p_dgeevx) return true;
  /* 1. an LP64 LAPACK in the global scope (e.g. R's own libRlapack) */
  if (lookup_lapack(RTLD_DEFAULT)) return true;
  /* 2. one this library was linked against (R loads package libraries
   *    RTLD_LOCAL, so e.g. PKG_LIBS = $(LAPACK_LIBS) is only visible through
   *    our own handle, which searches our dependency tree) */
  Dl_info self{};
  if (dladdr(reinterpret_cast<void *>(&pht_bind_lapack), &self) && self.dli_fname) {
    void *h = dlopen(self.dli_fname, RTLD_LAZY | RTLD_NOLOAD);
    if (h) {
      const bool ok = lookup_lapack(h);
      dlclose(h);
      if (ok) return true;
    }
  }
  /* 3. standalone: an explicit library (pht_bind_lapack or the environment) */
  const char *path = getenv("PHT_LAPACK_LIB");
  if (path) return pht_bind_lapack(path, getenv("PHT_LAPACK_PREFIX") ? getenv("PHT_LAPACK_PREFIX") : "") == 0;
  return false;
}

extern "C" int pht_bind_lapack(const char *path, const char *prefix) {
  void *h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (!h) {
    set_err("dlopen(%s): %s", path, dlerror());
    return 1;
  }
  const std::string pre = prefix ? prefix : "";
  if (!lookup_lapack(h, pre)) {
    set_err("LAPACK symbols %sdgeevx_/dgetrf_/dgetri_ not found in %s", pre.c_str(), path);
    return 2;
  }
  return 0;
}

static thread_local int g_blas_one = 0;
OneBlasThread::OneBlasThread() {
  if (g_blas_one++ == 0 && p_blas_threads) prev = p_blas_threads(1);
}
OneBlasThread::~OneBlasThread() {
  if (--g_blas_one == 0 && p_blas_threads && prev > 1) p_blas_threads(prev);
}

/* LAPACK workspace and scratch of eigen() per n, per host thread: the
 * workspace size is the reference's query result for that n (a pure function
 * of n), asked once instead of twice per sweep */
struct EigenWork {
  int n = -1, lw = 0;
  std::vector<double> A, evi, Ql, scl, rce, rcv, work;
  std::vector<int> iwork, ipiv;
};

/* LJMA_eigen with LJMA_Gibbs's workspace sizing (src/utility.c:87-129,
 * src/PHT_MCMC_Aslett.c:177-185). */
int pht::host::eigen(int n, const double *S, double *evals, double *Q, double *Qinv, double *evi_out) {
  OneBlasThread one;
  char balanc = 'B', jobv = 'V', sense = 'B';
  int lwork = -1, info = 0, ilo, ihi, nn = n;
  double wq = 0, abnrm;
  /* (a pointer: a thread_local object with a destructor left an undefined
   * EigenWork::~EigenWork in the shared library; one per thread, kept) */
  static thread_local EigenWork *ewp = nullptr;
  if (!ewp) ewp = new EigenWork;
  EigenWork &ew = *ewp;
  if (ew.n != n) {
    ew.A.assign(n * n, 0.0);
    ew.evi.assign(n, 0.0);
    ew.Ql.assign(n * n, 0.0);
    ew.scl.assign(n, 0.0);
    ew.rce.assign(n, 0.0);
    ew.rcv.assign(n, 0.0);
    ew.iwork.assign(2 * n + 2, 0);
    ew.ipiv.assign(n, 0);
    p_dgeevx(&balanc, &jobv, &jobv, &sense, &nn, ew.A.data(), &nn, evals, ew.evi.data(), ew.Ql.data(), &nn, Q, &nn,
             &ilo, &ihi, ew.scl.data(), &abnrm, ew.rce.data(), ew.rcv.data(), &wq, &lwork, nullptr, &info, 1, 1, 1, 1);
    int lw = (int)wq;
    p_dgetri(&nn, nullptr, &nn, nullptr, &wq, &lwork, &info);
    if ((int)wq > lw) lw = (int)wq;
    ew.lw = lw > 0 ? lw : 1;
    ew.work.assign(ew.lw, 0.0);
    ew.n = n;
  }
  int lw = ew.lw;
  double *A = ew.A.data(), *evi = ew.evi.data(), *work = ew.work.data();
  memcpy(A, S, sizeof(double) * n * n);
  /* The reference asks for condition numbers too (sense 'B'); they come
   * from dtrsna AFTER the eigenvectors and feed nothing it uses, so the
   * sweep skips them (sense 'N', same workspace as the 'B' query: the
   * Hessenberg/Schur/eigenvector arithmetic is unchanged — evals, Q and
   * Q^-1 stay bit-identical, tests/test_host.py).  That is most of the
   * per-sweep host time at n = 10. */
  char sense_n = 'N', jobvl_n = 'N';
  p_dgeevx(&balanc, &jobvl_n, &jobv, &sense_n, &nn, A, &nn, evals, evi, ew.Ql.data(), &nn, Q, &nn, &ilo,
           &ihi, ew.scl.data(), &abnrm, ew.rce.data(), ew.rcv.data(), work, &lw, ew.iwork.data(), &info, 1, 1, 1, 1);
  if (info != 0) {
    say("Error (LJMA_eigen 01): failed LAPACK call, code=%d\n", info);
    return info;
  }
  for (int i = 0; i < n; i++)
    if (evi[i] > 0) say("Error: imaginary part of eigenvalue %d found.\n", i + 1);
  if (evi_out) memcpy(evi_out, evi, sizeof(double) * n);
  memcpy(Qinv, Q, sizeof(double) * n * n);
  p_dgetrf(&nn, &nn, Qinv, &nn, ew.ipiv.data(), &info);
  if (info != 0) {
    say("Error (LJMA_inverse 01): failed LAPACK call, code=%d\n", info);
    return info;
  }
  p_dgetri(&nn, Qinv, &nn, ew.ipiv.data(), work, &lw, &info);
  if (info != 0) say("Error (LJMA_inverse 03): failed LAPACK call, code=%d\n", info);
  return info;
}

/* the device-mode spectral products of the packed block (explicit fma in
 * oracle/pht_oracle.c:orc_sp_build's order).  x86-64: a copy compiled with
 * hardware fma runs where the host has it (the baseline ISA's fma() is
 * glibc's software routine: half of build_params' time at n = 20); both are
 * correctly rounded, so the values are the same. */
static inline __attribute__((always_inline)) void spectral_products_body(int n, const double *S, const double *s,
                                                                         const double *P, const double *Q,
                                                                         const double *Qs, const double *Q1,
                                                                         double *d, const Layout &L) {
  double rj[kMaxN];
  for (int j = 0; j < n; j++) {
    const double Sjj = S[j + j * n];
    d[L.logs + j] = s[j] > 0.0 ? pht_log(s[j]) : 0.0;
    d[L.scale + j] = 1.0 / -Sjj;
    d[L.logscale + j] = pht_log(d[L.scale + j]);
    for (int k = 0; k < n; k++) rj[k] = S[j + k * n] / (-Sjj); /* hoisted: same quotients */
    for (int i = 0; i < n; i++) {
      double w = 0.0, v = 0.0;
      for (int k = 0; k < n; k++) {
        if (k != j) w = fma(rj[k], Q[k + i * n], w);
        v = fma(P[j + k * n], Q[k + i * n], v);
      }
      d[L.QQs + j + i * n] = Q[j + i * n] * Qs[i];
      d[L.W + j + i * n] = w * Qs[i];
      d[L.QQ1 + j + i * n] = Q[j + i * n] * Q1[i];
      d[L.V + j + i * n] = v * Q1[i];
    }
  }
  for (int i = 0; i < n; i++) {
    double a = 0.0;
    for (int k = 0; k < n; k++) a = fma(d[L.pi + k], Q[k + i * n], a);
    d[L.piQ + i] = a;
  }
  for (int j = 0; j < n; j++) { /* ECS starting point y_t - a (pht_detmath.h pht_wmoments) */
    double m[PHT_WMOM];
    pht_wmoments(n, d + L.W + j, n, d + L.evals, m);
    for (int k = 0; k < PHT_WMOM; k++) d[L.Wm + j + k * n] = m[k];
  }
}
#if defined(__x86_64__)
__attribute__((target("fma"))) static void spectral_products_fma(int n, const double *S, const double *s,
                                                                 const double *P, const double *Q, const double *Qs,
                                                                 const double *Q1, double *d, const Layout &L) {
  spectral_products_body(n, S, s, P, Q, Qs, Q1, d, L);
}
#endif
static void spectral_products(int n, const double *S, const double *s, const double *P, const double *Q,
                              const double *Qs, const double *Q1, double *d, const Layout &L) {
#if defined(__x86_64__)
  static const bool hw_fma = __builtin_cpu_supports("fma");
  if (hw_fma) {
    spectral_products_fma(n, S, s, P, Q, Qs, Q1, d, L);
    return;
  }
#endif
  spectral_products_body(n, S, s, P, Q, Qs, Q1, d, L);
}

/* ======================================================== sweep parameters */
/*
 * Packed per-sweep block (pht_layout.h) from (S, s): the embedded chain
 * exactly as src/PHT_MCMC_Aslett.c:279-297, the spectral data as :320-332
 * (Q⁻¹v by reference-BLAS dgemv order), and the device-mode products with
 * explicit fma in the order oracle/pht_oracle.c:orc_sp_build uses.
 */
int pht::host::build_params(int n, const double *S, const double *s, int method,
                            std::vector<unsigned char> &out) {
  const Layout L = make_layout(n);
  out.assign(L.bytes(), 0);
  double *d = reinterpret_cast<double *>(out.data());
  int *iv = reinterpret_cast<int *>(out.data() + L.ndouble * 8);
  double *P = d + L.P, *Pf = d + L.Pf, *Q = d + L.Q, *Qinv = d + L.Qinv, *ev = d + L.evals;
  memcpy(d + L.S, S, sizeof(double) * n * n);
  memcpy(d + L.s, s, sizeof(double) * n);
  d[L.pi + 0] = 1.0;
  for (int i = 0; i < n; i++) {
    double rsum, rsumfull = 0.0;
    for (int j = 0; j < n; j++) rsumfull += Pf[i + j * n] = P[i + j * n] = -S[i + j * n] / S[i + i * n];
    rsum = rsumfull - P[i + i * n];
    rsumfull += Pf[i + n * n] = -s[i] / S[i + i * n];
    rsumfull -= Pf[i + i * n];
    Pf[i + i * n] = P[i + i * n] = 0.0;
    for (int j = 0; j < n; j++) {
      P[i + j * n] = P[i + j * n] / rsum;
      Pf[i + j * n] = Pf[i + j * n] / rsumfull;
    }
    Pf[i + n * n] = Pf[i + n * n] / rsumfull;
  }
  std::vector<double> Qs(n, 0.0), Q1(n, 0.0);
  int info = 0;
  if (method & (kMethodECS | kMethodDCS)) {
    if (!lapack_ready()) {
      set_err("no LAPACK bound (call pht_bind_lapack or set PHT_LAPACK_LIB)");
      return -1;
    }
    info = eigen(n, S, ev, Q, Qinv);
    /* dgemv 'N' (reference BLAS order): y = 0; y += x[c] * A[:,c] */
    for (int c = 0; c < n; c++) {
      const double ts = 1.0 * s[c], t1 = 1.0 * 1.0;
      for (int r = 0; r < n; r++) {
        Qs[r] = Qs[r] + ts * Qinv[r + c * n];
        Q1[r] = Q1[r] + t1 * Qinv[r + c * n];
      }
    }
  }
  spectral_products(n, S, s, P, Q, Qs.data(), Q1.data(), d, L);
  for (int j = 0; j < n; j++) {
    int a = 0, b = 0, c = 0;
    for (int k = 0; k < n; k++) {
      if (!(P[j + k * n] == 0.0)) iv[L.succP + j * n + a++] = k;
      if (k != j && !(S[j + k * n] == 0.0)) iv[L.succS + j * n + c++] = k;
    }
    for (int k = 0; k <= n; k++)
      if (!(Pf[j + k * n] == 0.0)) iv[L.succPf + j * (n + 1) + b++] = k;
    iv[L.nsuccP + j] = a;
    iv[L.nsuccPf + j] = b;
    iv[L.nsuccS + j] = c;
  }
  return info;
}

extern "C" int pht_build_params(int n, const double *S, const double *s, int method, unsigned char *out,
                                int out_bytes) {
  std::vector<unsigned char> v;
  int info = build_params(n, S, s, method, v);
  if (info < 0) return info;
  if ((int)v.size() > out_bytes) return -2;
  memcpy(out, v.data(), v.size());
  return info;
}
extern "C" int pht_params_bytes(int n) { return make_layout(n).bytes(); }
extern "C" int pht_stats_len(int n) { return stats_len(n); }
