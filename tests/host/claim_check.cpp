/*
 * Stand-alone check of the persistent kernels' claim arithmetic
 * (phasetype_amd/csrc/pht_claim.h): the equal stripes (claim_pos) and the
 * weighted dealing between the two blocks of a CU (pair_pos).  For every
 * grid, ratio and chunk count, with a ragged last chunk: every position of
 * the range is claimed exactly once, a block's positions increase with its
 * claim index (a lane stops at its first position past the range), and over
 * whole stripes blocks b and b + h take chunks in the ratio P : Q.
 */
#include <stdio.h>

#include <vector>

#include "pht_claim.h"

using namespace pht;

static int g_fail = 0;
#define CHECK(c, ...)                   \
  do {                                  \
    if (!(c)) {                         \
      printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);              \
      printf("\n");                     \
      g_fail++;                         \
    }                                   \
  } while (0)

/* mode 0: claim_pos over grid blocks; otherwise pair_claim(mode) with h = grid / 2 */
static void run(int mode, unsigned grid, long nch, long ragged) {
  const long count = nch > 0 ? nch * kClaimChunk - ragged : 0;
  std::vector<int> seen((size_t)count, 0);
  std::vector<long> chunks(grid, 0);
  for (unsigned b = 0; b < grid; b++) {
    long prev = -1;
    /* far enough past the range to see that positions keep increasing */
    const long tmax = (nch / grid + 9) * 8 * kClaimChunk;
    bool past = false;
    for (long t = 0; t < tmax; t++) {
      const long p = mode ? pair_claim(mode, (unsigned)t, b, grid / 2) : claim_pos(t, b, grid);
      CHECK(p > prev, "mode %d grid %u block %u: position %ld after %ld at t = %ld", mode, grid, b, p, prev, t);
      prev = p;
      if (p >= count) {
        past = true;
        continue;
      }
      CHECK(!past, "mode %d grid %u block %u: position %ld inside the range after one past it", mode, grid, b, p);
      /* a chunk's positions are consecutive: the ragged last chunk keeps its place */
      CHECK(p % kClaimChunk == t % kClaimChunk, "mode %d: offset %ld of claim %ld", mode, p % kClaimChunk, t);
      seen[(size_t)p]++;
      if (t % kClaimChunk == 0) chunks[b]++;
    }
    CHECK(past, "mode %d grid %u block %u: never left the range", mode, grid, b);
  }
  long bad = 0;
  for (long p = 0; p < count; p++) bad += seen[(size_t)p] != 1;
  CHECK(bad == 0, "mode %d grid %u chunks %ld: %ld positions not claimed exactly once", mode, grid, nch, bad);
  if (mode) {
    const int P = mode / 10, Q = mode % 10;
    const unsigned h = grid / 2;
    const long stripes = nch / ((long)(P + Q) * h), rest = nch % ((long)(P + Q) * h);
    for (unsigned b = 0; b < h; b++) {
      /* whole stripes give P and Q chunks; the last, partial one at most that */
      CHECK(chunks[b] >= stripes * P && chunks[b] <= (stripes + (rest > 0)) * P, "mode %d block %u: %ld chunks", mode, b,
            chunks[b]);
      CHECK(chunks[b + h] >= stripes * Q && chunks[b + h] <= (stripes + (rest > 0)) * Q, "mode %d block %u: %ld chunks",
            mode, b + h, chunks[b + h]);
    }
  }
}

int main() {
  const int modes[] = {0, 32, 43};
  const unsigned grids[] = {1, 2, 4, 512};
  for (int mode : modes)
    for (unsigned grid : grids) {
      if (mode && (grid & 1)) continue;
      const long nchs[] = {0, 1, (long)grid - 1, grid, (long)grid + 1, 4L * grid, 30L * grid + 7, 15625};
      for (long nch : nchs) {
        if (nch < 0) continue;
        run(mode, grid, nch, 0);
        if (nch > 0) run(mode, grid, nch, 37);
      }
    }
  CHECK(pair_mode_ok(43) && pair_mode_ok(32) && !pair_mode_ok(75) && !pair_mode_ok(0) && !pair_mode_ok(1) &&
            !pair_mode_ok(21),
        "pair_mode_ok");
  if (g_fail) {
    printf("claim arithmetic: %d failures\n", g_fail);
    return 1;
  }
  printf("claim arithmetic: ok\n");
  return 0;
}
