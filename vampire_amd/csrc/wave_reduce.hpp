// The fixed-order sums of the loss, target and detection kernels (float64 partials added in one
// order, so every result is bitwise repeatable): a butterfly over the 64 lanes of a wave, then the waves in index order.
#pragma once
#include <hip/hip_runtime.h>

namespace vamp {

// sum over the wave's 64 lanes (xor butterfly from 32 down to 1); every lane holds it afterwards
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over a workgroup of WAVES waves: butterfly per wave, then thread 0 adds the waves in order.  Valid in thread 0
// only; `red` (WAVES elements of LDS) is free again on return.  Every thread of the workgroup must call it.
template <int WAVES, typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  T tot = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < WAVES; ++w) tot += red[w];
  __syncthreads();
  return tot;
}

}  // namespace vamp
