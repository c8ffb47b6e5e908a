/* pht_wave.h — a value summed over the 64 lanes of a wavefront by a butterfly
 * of shuffles, in every lane (double: pht_psis_butterfly's order, pht_psis.h) */
#ifndef PHT_WAVE_H
#define PHT_WAVE_H

#include <hip/hip_runtime.h>

namespace pht {

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

}  // namespace pht

#endif
