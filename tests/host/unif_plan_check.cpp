/*
 * Stand-alone check of phasetype_amd/csrc/host_unif_plan.h (no HIP, no
 * library): the plan of a call of the uniformisation analyses over draws of
 * n = 3 whose largest rates differ by 40 (so K differs within a batch) and one
 * draw with a NaN entry, for 1, 5 and 65 draws in batches of 1, 2 and 64: the
 * meta words against direct pht_llu_meta calls bit for bit, the flagged draw,
 * Kcall and the stride, Kmax of every batch (the short last one included), the
 * tiling of the input buffer, a callback that flags a draw of its own, and a
 * null flags_out.  Built and run by tests/test_unif_plan.py, with the address
 * and undefined-behaviour sanitizers where the compiler has them.
 */
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "host_unif_plan.h"

using pht::host::UnifPlan;

static int g_bad = 0;
#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);  \
      g_bad++;                                                    \
    }                                                             \
  } while (0)

static const int kN = 3;
static const double kYmax = 7.5;
static const unsigned kOwnFlag = 64u; /* an analysis' own flag bit (the condition's trap flag) */

/* draw d: a 3-state generator (column-major) at scale 1 (even d) or 40 (odd
 * d), a little different for every d; nan_at: that draw has a NaN entry */
static void draws(int nd, int nan_at, std::vector<double> &S, std::vector<double> &s) {
  S.assign((size_t)nd * kN * kN, 0.0);
  s.assign((size_t)nd * kN, 0.0);
  for (int d = 0; d < nd; d++) {
    const double sc = ((d & 1) ? 40.0 : 1.0) * (1.0 + 0.001 * d);
    double *Sd = S.data() + (size_t)d * kN * kN, *sd = s.data() + (size_t)d * kN;
    const double rows[3][4] = {{-3.0, 2.0, 0.5, 0.5}, {0.25, -2.0, 1.0, 0.75}, {0.0, 0.5, -1.5, 1.0}};
    for (int i = 0; i < kN; i++) {
      for (int j = 0; j < kN; j++) Sd[i + j * kN] = sc * rows[i][j];
      sd[i] = sc * rows[i][3];
    }
    if (d == nan_at) Sd[1 + 2 * kN] = std::nan("");
  }
}

static void one_case(int nd, int batch) {
  const int nan_at = nd >= 5 ? nd / 2 : -1;
  std::vector<double> S, s;
  draws(nd, nan_at, S, s);
  std::vector<int> flags(nd, -1);
  const auto plain = [&](int, const double *Sd, const double *sd, double *m) {
    return pht_llu_meta(kN, Sd, sd, kYmax, m);
  };
  const UnifPlan p(kN, nd, S.data(), s.data(), batch, flags.data(), plain);

  /* every word against a direct call; Kcall over the unflagged draws */
  std::vector<int> K(nd, 0);
  int Kcall = 0, Klo = PHT_LLU_MAXK, Khi = 0;
  CHECK(p.meta.size() == (size_t)nd * PHT_LLU_META);
  for (int d = 0; d < nd; d++) {
    double m[PHT_LLU_META];
    const unsigned flag = pht_llu_meta(kN, S.data() + (size_t)d * kN * kN, s.data() + (size_t)d * kN, kYmax, m);
    CHECK(std::memcmp(m, p.meta.data() + (size_t)d * PHT_LLU_META, sizeof m) == 0);
    CHECK(flags[d] == (int)flag);
    CHECK(p.flagged(d) == (flag != 0));
    CHECK((d == nan_at) == (flag != 0));
    K[d] = (int)m[PHT_LLU_M_K];
    CHECK(p.K(d) == K[d]);
    if (flag) {
      CHECK(K[d] == 0);
      continue;
    }
    Kcall = std::max(Kcall, K[d]);
    Klo = std::min(Klo, K[d]);
    Khi = std::max(Khi, K[d]);
  }
  CHECK(Khi < PHT_LLU_MAXK); /* nothing at the cap: the lengths are the draws' own */
  if (nd > 1) CHECK(Khi > 4 * Klo); /* mixed table lengths */
  CHECK(p.Kcall == Kcall);
  CHECK(p.stride == 2 * (Kcall + 1));
  CHECK(p.bmax == std::min(batch, nd));
  CHECK(p.tab_doubles() == (size_t)p.bmax * p.stride);

  /* Kmax of exactly each batch */
  int nbatches = 0;
  for (int d0 = 0; d0 < nd; d0 += batch, nbatches++) {
    const int nb = std::min(batch, nd - d0);
    int want = 0;
    for (int d = d0; d < d0 + nb; d++) want = std::max(want, K[d]);
    CHECK(p.Kmax(d0, nb) == want);
  }
  CHECK(nbatches == (nd + batch - 1) / batch);

  /* [S | s | meta] tile the input buffer */
  CHECK(p.nS == (size_t)nd * kN * kN && p.ns == (size_t)nd * kN);
  CHECK(p.off_S() == 0);
  CHECK(p.off_s() == p.off_S() + p.nS);
  CHECK(p.off_meta() == p.off_s() + p.ns);
  CHECK(p.in_doubles() == p.off_meta() + p.meta.size());

  /* a callback with a flag of its own on draw `own` (the condition's case):
   * its words are zero, the flag is in word 0, Kcall is the others' */
  const int own = nd - 1;
  const auto flagging = [&](int d, const double *Sd, const double *sd, double *m) {
    unsigned flag = pht_llu_meta(kN, Sd, sd, kYmax, m);
    if (!flag && d == own) {
      flag = kOwnFlag;
      m[PHT_LLU_M_FLAG] = pht_u2d((uint64_t)flag);
      m[PHT_LLU_M_MU] = m[PHT_LLU_M_ABAR] = m[PHT_LLU_M_K] = 0.0;
    }
    return flag;
  };
  std::fill(flags.begin(), flags.end(), -1);
  const UnifPlan q(kN, nd, S.data(), s.data(), batch, flags.data(), flagging);
  const double *mo = q.meta.data() + (size_t)own * PHT_LLU_META;
  CHECK(pht_d2u(mo[PHT_LLU_M_FLAG]) == kOwnFlag);
  CHECK(mo[PHT_LLU_M_MU] == 0.0 && mo[PHT_LLU_M_ABAR] == 0.0 && mo[PHT_LLU_M_K] == 0.0);
  CHECK(flags[own] == (int)kOwnFlag && q.flagged(own) && q.K(own) == 0);
  int Kothers = 0;
  for (int d = 0; d < nd; d++) {
    if (d != own) Kothers = std::max(Kothers, K[d]);
    if (d != own) CHECK(flags[d] == (d == nan_at ? (int)PHT_LL_F_NONFINITE : 0));
  }
  CHECK(q.Kcall == Kothers && q.stride == 2 * (Kothers + 1));

  /* no flags_out */
  const UnifPlan r(kN, nd, S.data(), s.data(), batch, nullptr, plain);
  CHECK(r.meta == p.meta && r.Kcall == p.Kcall && r.stride == p.stride);
}

int main() {
  for (int nd : {1, 5, 65})
    for (int batch : {1, 2, 64}) one_case(nd, batch);
  if (g_bad) return 1;
  std::printf("unif plan: ok\n");
  return 0;
}
