/*
 * pht_claim.h — which positions of a launch range a block of a persistent
 * kernel claims: pure index arithmetic, shared by the kernels
 * (pht_kernels_impl.h) and the stand-alone host check (tests/host/).
 */
#ifndef PHT_CLAIM_H
#define PHT_CLAIM_H

#if defined(__HIPCC__)
#define PHT_CLAIM_FN __host__ __device__ __forceinline__
#else
#define PHT_CLAIM_FN inline
#endif

namespace pht {

/* Position of a block's t-th claim in the persistent kernels: chunks of
 * kClaimChunk consecutive positions, block b taking chunks b, b + grid, ...
 * (the sorted order is walked by all blocks together; a wavefront's claims
 * are contiguous, so its y/gid loads coalesce).  Increasing in t. */
constexpr int kClaimChunk = 64;
PHT_CLAIM_FN long claim_pos(long t, unsigned blk, unsigned nblk) {
  return ((t / kClaimChunk) * (long)nblk + blk) * kClaimChunk + (t % kClaimChunk);
}

/* The ECS exact kernel's weighted dealing between the two blocks of a CU.
 * With a grid of two blocks per CU, blocks b and b + h (h = half the grid)
 * share a CU, and the SIMDs issue the older wave first: block b runs its
 * rounds at nearly the speed of a lone block and block b + h takes what is
 * left, about half of that, until b ends.  Equal shares
 * therefore leave every SIMD with one wave for the last quarter of the
 * kernel.  Here a stripe is (P + Q) h chunks: its first P h go to blocks
 * [0, h) (block b: chunks b, b + h, ...), its last Q h to blocks [h, 2h), so
 * both blocks of a CU walk the sorted order at the pace they run at and end
 * together.  Every chunk belongs to exactly one block; increasing in t. */
template <int P, int Q>
PHT_CLAIM_FN long pair_pos(unsigned t, unsigned blk, unsigned h) {
  const unsigned k = t / kClaimChunk, r = t % kClaimChunk;
  /* (a block-uniform branch: each side divides by its constant) */
  long c;
  if (blk < h) c = (long)(k / P) * (long)((P + Q) * h) + (long)((k % P) * h + blk);
  else c = (long)(k / Q) * (long)((P + Q) * h) + (long)((P + k % Q) * h + (blk - h));
  return c * kClaimChunk + r;
}
/* mode = 10 P + Q (SweepArgs::pair, PHT_ECS_PAIR): the ratios built */
PHT_CLAIM_FN bool pair_mode_ok(int mode) { return mode == 43 || mode == 32; }
PHT_CLAIM_FN long pair_claim(int mode, unsigned t, unsigned blk, unsigned h) {
  switch (mode) {
    case 32: return pair_pos<3, 2>(t, blk, h);
    default: return pair_pos<4, 3>(t, blk, h);
  }
}

}  // namespace pht

#endif
